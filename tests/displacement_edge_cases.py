"""Displacement (pysdm_amd/csrc/displacement.hip, pysdm_amd/displacement.py) against a NumPy
restatement of one `Displacement.__call__`, at cell faces, at the precipitation level, at the top
of the column and past one pass of the precipitation kernel's grid; and the two fall-velocity laws
against NumPy at their knots and regime limits.  Written once and run with the oracle engine (CPU)
and the HIP engine (GPU); the oracle is a second system under test, not the reference.

Why the comparison is exact.  Both libraries are built without contraction and the per-row
arithmetic is plain IEEE double, so `reference_step` (NumPy, vectorised over super-droplets, the
compactions taken from tests/index_cases.py) must agree to the bit, positions included (compared as
uint64: the sign of a zero counts).  The fall velocity is no part of that reference: it is
downloaded from the engine under test before each call and fed to it.  Masses are j * 2^-40 kg
with j < 2^19 and multiplicities are below 8, so every sum of |m| * n over fewer than 2^20 rows is
exact in any order and the rainfall is compared with ==, although the GPU adds in wave-tree order.

How the edges are reached.  Positions and Courant numbers are integers / 1024, dt and the cell
sizes powers of two.  A planted row sits in a cell whose two faces along the row's axis carry the
same Courant number c: c (1 - x) + c x is then c exactly, under both schemes (1 - c + c is 1), and
a row of mass 0 has fall velocity 0 (the table's first value), so that x + v is the value wanted,
exactly.  Rows whose mass must be counted carry a small mass (j <= 11: they fall far less than a
cell) and classes that do not need an exact landing.  Rows planted along the periodic axis 0 sit in
cells whose vertical faces carry 0, at mid-height: they stay in the column and are compared after
the step.  `_assert_planted` checks on the reference's intermediate values that every class of a
case is present, landed where it was aimed and met its fate; no case passes with a class empty.

The classes (name: where it lands after the first sub-step -> fate).  Along axis 0 (periodic):
carry1, carry2: x + v == 1.0, 2.0 -> carried, new position +0.0; zero+: == +0.0; zero-: == -0.0
(faces -0.0 / +0.0, x = -0.0: the position keeps its sign bit); below0, below0tiny: -1/1024 and
-2^-54 from origin 0 (negative floor, Python's %; the second one's new position rounds to 1.0);
neg1: -1.0; neg275: -2.75.  Along the last axis: top: z == top -> stays, wraps to origin 0; top+:
one ulp above -> out; level=: z == level with v < 0 (z == 0.0 moving down for level 0) -> stays;
level-: one ulp below (-2^-54 for level 0) -> rain; below,v=0 / below,v>0 / below,v=-0: in the
lowest cell with v == 0.0, > 0, == -0.0 -> stay; precedence: z < 0 and v < 0 -> rain with its mass
counted, out of column (nothing counted) without sedimentation; two-cells: through two whole
cells and the level in one sub-step; again: rain in sub-step 1 and classified as rain again in
sub-step 2 (adaptive, level >= 1): counted once; dead: multiplicity 0 from before the call, on the
trajectory of `precedence`, outside perm[:live]: adds nothing.

A grid with one column (1-D, or extent 1 along axis 0) has three independent cells along the last
axis and carries the classes that fit; the size sweep below 320 rows plants as many rows as it has
(the first of them `precedence`: at size 1 the only row rains), from 320 rows on every class has
four rows in four different wavefronts of the permutation.  The adaptive case carries the classes
that sub-stepping is about: an exact landing after sub-step 1 is moved on by sub-steps 2 to 4.

Constants of the kernels and the case that crosses each:

  constant                        where                      crossed by
  SDM_WAVE = 64 (shuffle tree)    displacement.hip:80, :313  sizes 63 / 64 / 65
  SDM_BLOCK = 256 (one partial    displacement.hip:66, :290  sizes 255 / 256 / 257, every case of
  per workgroup)                                             549 rows (three workgroups)
  strict comparisons of the two   displacement.hip:73, :149, level=, level-, top, top+, precedence
  removals, their precedence      :254-258                   (with and without sedimentation)
  floor, Python's %               displacement.hip:269-273   below0, below0tiny, neg1, neg275 on
                                                             extents 1, 2 and 7
  face extents grid[d] + (d ==    displacement.hip:238-240,  grid (2, 3, 4): all extents differ
  dim) of l and r                 :24-28
  Courant / n_substeps,           displacement.hip:243,      the adaptive case (4 sub-steps)
  dt / n_substeps / dz            displacement.py:116, :181
  DISP_PRECIP_GRID = 1024         displacement.hip:288-294,  262144 (one pass, the last such size),
  workgroups, then a stride loop  :381                       262145 (the first with a stride),
                                                             262401 = 1026 workgroups (two passes
                                                             and a tail; rain planted at positions
                                                             262144, 262399 and 262400)
  1024 threads fold the partials  displacement.hip:92-107    the same three sizes (1024 partials)
  compaction: serial reference    index_cases.py:SERIAL_MAX  262145 and 262401 use the closed form
  up to 2^18
  601 table points, r_id clamp    physics.h:30-40            interpolation at every knot, one ulp
                                                             either side, 0, 6 mm, r < 0
  strict regime limits            collisions.hip:829         Rogers-Yau at both limits +- one ulp

What was tried against these cases (single edits on a scratch copy, never committed).  Edits of
the oracle, and the oracle tests that then fail (`size-1` has one row, `precedence`, and notices
only the swapped precedence):
  `<= level` in flag_precipitated: every case with `level=` and sedimentation - all but size-1,
    2d-dry and adaptive, both routes.
  `>= top` in flag_out_of_column: every case with `top` - all but size-1, extent1 and adaptive.
  trunc for floor (fused step and sdm_floor_to_i64): every case but size-1.
  C's % for the periodic wrap (fused step; the MOD of sdm_elementwise_i64 for the chain): the
    fused, or the chain, tests of every 2-D and 3-D case but size-1 and extent1 (anything % 1
    is 0; in 1-D a negative origin belongs to a removed row).
  out of column tested before precipitation (fused step; the chain's order is host code): the
    fused tests of every case with sedimentation, size-1 included.
  Courant not divided by n_substeps: the adaptive case alone, both routes.
  dt / dz for dt / n_substeps / dz (fused step; the chain's factor is host code): adaptive, fused.
  r built without + (d == dim) in the extent: every 2-D and 3-D case but size-1.
Edits of displacement.hip.  Two keep every access in bounds and were built: k_fold_partials
reading n - 1 partials, and `cls` written before the sedimentation term is applied; no GPU was to
be had when this was written, so they have not been run against these cases.  The third, a
k_disp_precip stride of (gridDim.x - 1) * SDM_BLOCK, was not tried: with one workgroup the stride
is 0 and the loop never ends, and beyond one pass the positions visited twice are read again after
they were flagged, idx[i] == n_sd, which indexes one past `cls` and the columns.
"""
import functools
import itertools

import numpy as np

from pysdm_amd.displacement import DisplacementRunner, substeps_for
from pysdm_amd.engine import FLOAT
from pysdm_amd.population import Population, grid_strides
from pysdm_amd.terminal_velocity import (TABLE_POINTS_PER_METRE, TABLE_TOP, RogersYau,
                                         gunn_kinzer_table)

from .index_cases import SERIAL_MAX, Case, compact_closed_form, compact_serial

UNIT = 1024            # positions and Courant numbers are integers / UNIT
MASS_UNIT = 2.0**-40   # kg; masses are j * MASS_UNIT
J_MAX = 2**19          # radius below 0.49 mm: inside the Gunn-Kinzer table
DZ = 64.0              # m; every cell
DT_OVER_DZ = 0.5       # per sub-step: the largest drops (4 m/s) fall two cells, the smallest 0.002
PASS = 1024 * 256      # positions one pass of k_disp_precip covers
EXPLICIT, IMPLICIT = "ExplicitInSpace", "ImplicitInSpace"


def bits(value):
    return np.asarray(value, dtype=np.float64).view(np.uint64)


# ---- the reference ------------------------------------------------------------------------------
def _compact(perm, mult, live, n_sd):
    return (compact_serial if live <= SERIAL_MAX else compact_closed_form)(perm, mult, live, n_sd)


def reference_step(state, cfg, fall, trace=None):
    """one `DisplacementRunner.run()` on plain arrays.  `state`: perm, live, origin (D, N) int64,
    pos (D, N) float64 - replaced by the new ones in the returned dict; `cfg`: a Case with grid,
    scheme, sed, level, n_substeps, dt, courant, mult, mass.  `trace`, a list, receives one dict
    per sub-step with the intermediate values the host assertions read"""
    grid, dims = cfg.grid, len(cfg.grid)
    n_sd = cfg.mult.shape[0]
    n_sub = cfg.n_substeps
    perm, live = state["perm"].copy(), int(state["live"])
    origin, pos = state["origin"].copy(), state["pos"].copy()
    strides = grid_strides(grid).reshape(-1, 1)
    rain = 0.0
    for _ in range(n_sub):
        disp = np.empty_like(pos)
        for dim in range(dims):  # all from the positions before the move
            left = tuple(origin[d] for d in range(dims))
            right = tuple(origin[d] + (1 if d == dim else 0) for d in range(dims))
            c_l = cfg.courant[dim][left] / float(n_sub)
            c_r = cfg.courant[dim][right] / float(n_sub)
            x = pos[dim]
            v = c_l * (1 - x) + c_r * x
            if cfg.scheme == IMPLICIT:
                v = v / (1 - c_r + c_l)
            disp[dim] = v
        if cfg.sed:
            k = cfg.dt / n_sub / DZ
            v = disp[-1]
            v = v * (1 / k)
            v = v - fall
            v = v * k
            disp[-1] = v
        pos = pos + disp
        z = origin[-1].astype(np.float64) + pos[-1]
        step = {"landed": pos.copy(), "z": z, "disp": disp, "alive": perm[:live].copy(),
                "rained": np.empty(0, dtype=np.int64), "rain_positions": np.empty(0, np.int64)}
        if cfg.sed:
            ids = perm[:live]
            hit = (disp[-1][ids] < 0) & (z[ids] < cfg.level)
            step["rained"], step["rain_positions"] = ids[hit], np.flatnonzero(hit)
            rain += float(np.sum(np.abs(cfg.mass[ids[hit]]) * cfg.mult[ids[hit]].astype(float)))
            if hit.any():
                perm[:live][hit] = n_sd
                perm, live = _compact(perm, cfg.mult, live, n_sd)
        ids = perm[:live]
        gone = (z[ids] < 0) | (z[ids] > float(grid[-1]))
        step["left"] = ids[gone]
        if gone.any():
            perm[:live][gone] = n_sd
            perm, live = _compact(perm, cfg.mult, live, n_sd)
        whole = np.floor(pos).astype(np.int64)
        origin = origin + whole
        pos = pos - whole.astype(np.float64)
        for d in range(dims):
            origin[d] %= grid[d]
        if trace is not None:
            trace.append(step)
    return {"perm": perm, "live": live, "origin": origin, "pos": pos,
            "cell_id": (origin * strides).sum(axis=0), "rain": rain}


# ---- the planted classes ------------------------------------------------------------------------
class Spec:  # pylint: disable=too-few-public-methods,too-many-instance-attributes
    """a class of planted rows: along `axis` ('h': axis 0, 'z': the last) from cell `o` at
    position x, the faces of its cell at c (or (c_l, c_r)); `land`: x + v after the first
    sub-step, to the bit (None: not aimed)"""

    def __init__(self, name, axis, o, x, c, fate, land=None, j=0, n=1):
        self.name, self.axis, self.o, self.x, self.fate, self.land = name, axis, o, x, fate, land
        self.faces = c if isinstance(c, tuple) else (c, c)
        self.j, self.n = j, n


def catalog(grid, level, sed):
    top = grid[-1]
    far = 2 if grid[0] > 2 else 0
    top_ulp = float(np.nextafter(float(top), np.inf)) - top
    level_ulp = level - float(np.nextafter(float(level), -np.inf)) if level > 0 else 2.0**-54
    wet = "rain" if sed else "out"
    specs = (
        Spec("carry1", "h", far, 0.5, 0.5, "stay", 1.0),
        Spec("carry2", "h", far, 0.5, 1.5, "stay", 2.0),
        Spec("zero+", "h", 0, 0.25, -0.25, "stay", 0.0),
        Spec("zero-", "h", far, -0.0, (-0.0, 0.0), "stay", -0.0),
        Spec("below0", "h", 0, 0.25 - 1 / UNIT, -0.25, "stay", -1 / UNIT),
        Spec("below0tiny", "h", 0, 0.25 - 2.0**-54, -0.25, "stay", -(2.0**-54)),
        Spec("neg1", "h", 0, 0.25, -1.25, "stay", -1.0),
        Spec("neg275", "h", 0, 0.25, -3.0, "stay", -2.75),
        Spec("top", "z", top - 1, 0.5, 0.5, "stay", 1.0),
        Spec("top+", "z", top - 1, 0.5 + top_ulp, 0.5, "out", 1.0 + top_ulp),
        Spec("level=", "z", level, 0.25, -0.25, "stay", 0.0),
        Spec("level-", "z", level, 0.25 - level_ulp, -0.25,
             "rain" if sed else ("out" if level == 0 else "stay"), -level_ulp),
        Spec("below,v=0", "z", 0, 0.5, 0.0, "stay", 0.5),
        Spec("below,v>0", "z", 0, 0.125, 0.5, "stay", 0.625),
        Spec("below,v=-0", "z", 0, 0.5, -0.0, "stay", 0.5),
        Spec("precedence", "z", 0, 0.125, -0.25, wet, j=5, n=3),
        Spec("two-cells", "z", 2, 0.25, -2.5, wet, j=7, n=2),
        Spec("again", "z", level, 0.125, -0.25, "rain", j=11, n=1),
        Spec("dead", "z", 0, 0.125, -0.25, "dead", j=9, n=0),
    )
    return {spec.name: spec for spec in specs}


HORIZONTAL = ("zero+", "below0", "below0tiny", "neg275", "neg1", "carry1", "carry2", "zero-")
VERTICAL = ("precedence", "level=", "level-", "top", "top+", "two-cells", "dead", "below,v=0",
            "below,v>0", "below,v=-0")
ALL_CLASSES = VERTICAL[:7] + HORIZONTAL + VERTICAL[7:]
ONE_COLUMN_1D = ("precedence", "level=", "level-", "top", "top+", "two-cells", "dead")
ONE_COLUMN_2D = ("precedence", "level=", "level-", "two-cells", "dead", "zero+", "below0",
                 "below0tiny", "neg275")
ADAPTIVE = ("precedence", "two-cells", "again", "dead")
LARGE = tuple(cls for cls in ALL_CLASSES if cls != "dead")  # (perm stays the identity)
FULL_FROM = 320  # rows from which every class has four rows in four wavefronts

# name: (n_sd, grid, scheme, sedimentation, level, adaptive, largest |C| of the random faces,
#        classes)
SIZES = (1, 63, 64, 65, 255, 256, 257)
CASES = {f"size-{n}": (n, (7, 3), EXPLICIT, True, 1, False, 2.9, ALL_CLASSES) for n in SIZES}
CASES.update({
    "1d": (549, (5,), EXPLICIT, True, 0, False, 2.9, ONE_COLUMN_1D),
    "extent1": (549, (1, 6), EXPLICIT, True, 0, False, 2.9, ONE_COLUMN_2D),
    "2d-explicit": (549, (7, 3), EXPLICIT, True, 2, False, 2.9, ALL_CLASSES),
    "2d-implicit": (549, (7, 3), IMPLICIT, True, 1, False, 0.45, ALL_CLASSES),
    "2d-dry": (549, (7, 3), EXPLICIT, False, 0, False, 2.9, ALL_CLASSES),
    "3d": (549, (2, 3, 4), EXPLICIT, True, 1, False, 2.9, ALL_CLASSES),
    "adaptive": (549, (2, 3, 4), IMPLICIT, True, 2, True, 0.35, ADAPTIVE),
    "two-passes": (PASS + 257, (7, 3), EXPLICIT, True, 1, False, 2.9, LARGE),
})
STEP_CASES = tuple(CASES)  # two steps, both routes
# one step, fused route only: the last size with one pass and the first with a stride
CASES.update({
    "one-pass": (PASS, (7, 3), EXPLICIT, True, 1, False, 2.9, LARGE),
    "first-stride": (PASS + 1, (7, 3), EXPLICIT, True, 1, False, 2.9, LARGE),
})
EDGE_CASES = ("one-pass", "first-stride")
ADAPTIVE_SUBSTEPS = 4


class _Field:
    """the Courant field of a case: random integers / UNIT, and the faces planted into it"""

    def __init__(self, rng, grid, c_max, whole_lines):
        self.grid, self.whole_lines = grid, whole_lines
        bound = int(c_max * UNIT)
        self.faces = [rng.integers(-bound, bound + 1, tuple(
            g + (1 if a == d else 0) for a, g in enumerate(grid))).astype(np.float64) / UNIT
                      for d in range(len(grid))]
        self.planted = [np.zeros(f.shape, dtype=bool) for f in self.faces]
        self.hosts = {}

    def _wanted(self, component, cell, c_l, c_r):
        """(index, value) of the faces to set: the cell's two, or its whole line"""
        if not self.whole_lines:
            right = tuple(o + (1 if d == component else 0) for d, o in enumerate(cell))
            return [(cell, c_l), (right, c_r)]
        assert bits(c_l) == bits(c_r)
        return [(tuple(f if d == component else o for d, o in enumerate(cell)), c_l)
                for f in range(self.grid[component] + 1)]

    def _fits(self, component, wanted):
        return all(not self.planted[component][index]
                   or bits(self.faces[component][index]) == bits(value)
                   for index, value in wanted)

    def host(self, spec, scale):
        """a cell for the rows of `spec`, found once per (axis, cell along it, faces)"""
        dims = len(self.grid)
        axis = 0 if spec.axis == "h" else dims - 1
        c_l, c_r = (c * scale for c in spec.faces)
        key = (axis, spec.o, int(bits(c_l)), int(bits(c_r)))
        if key in self.hosts:
            return self.hosts[key]
        others = [range(g) for d, g in enumerate(self.grid) if d != axis]
        choices = list(itertools.product(*others))
        for rest in (reversed(choices) if spec.axis == "h" else choices):
            cell = list(rest)
            cell.insert(axis, spec.o)
            cell = tuple(cell)
            sets = [(axis, self._wanted(axis, cell, c_l, c_r))]
            if spec.axis == "h":  # at rest in the vertical: the row stays in the column
                sets.append((dims - 1, self._wanted(dims - 1, cell, 0.0, 0.0)))
            if all(self._fits(component, wanted) for component, wanted in sets):
                for component, wanted in sets:
                    for index, value in wanted:
                        self.faces[component][index] = value
                        self.planted[component][index] = True
                self.hosts[key] = cell
                return cell
        raise AssertionError(f"no cell left for class {spec.name} on grid {self.grid}")


def _substep_rtol(courant):
    """an rtol at which substeps_for gives ADAPTIVE_SUBSTEPS: between the worst relative
    differences at half as many and at that many sub-steps (displacement.py:26-38)"""
    def worst(count):
        steps = [np.amax(np.abs(np.diff(c, axis=a))) / count for a, c in enumerate(courant)]
        return max(0.0 if s == 0 else 1 / (1 / s - 1) for s in steps)
    low, high = worst(ADAPTIVE_SUBSTEPS), worst(ADAPTIVE_SUBSTEPS // 2)
    assert 0 < low < high and all(worst(c) >= high for c in (1, 2))
    return (low + high) / 2


@functools.lru_cache(maxsize=3)
def make_case(name):  # pylint: disable=too-many-locals,too-many-statements
    n_sd, grid, scheme, sed, level, adaptive, c_max, classes = CASES[name]
    rng = np.random.default_rng([7] + [ord(ch) for ch in name])
    dims = len(grid)
    scale = ADAPTIVE_SUBSTEPS if adaptive else 1
    field = _Field(rng, grid, c_max, whole_lines=adaptive)
    origin = np.stack([rng.integers(0, g, n_sd) for g in grid]).astype(np.int64)
    pos = rng.integers(0, UNIT, (dims, n_sd)).astype(np.float64) / UNIT
    # masses spread over the decades: drops that hardly fall beside drops that fall two cells
    j = np.exp2(rng.uniform(0, 19, n_sd)).astype(np.int64)
    j[rng.integers(0, n_sd, n_sd // 8)] = J_MAX - 1
    mult = rng.integers(1, 8, n_sd).astype(np.int64)
    specs = catalog(grid, level, sed)
    stride = max(n_sd // 4, len(classes)) if n_sd >= FULL_FROM else len(classes)
    # (below FULL_FROM rows at most half of them are planted ones, but every class once if it fits)
    limit = n_sd if n_sd >= FULL_FROM else min(n_sd, max(len(classes), n_sd // 2))
    planted = [(copy * stride + q, specs[cls]) for copy in range(4)
               for q, cls in enumerate(classes) if copy * stride + q < limit]
    if n_sd > PASS:  # rain at the first and the last position of the second pass and its tail
        taken = {row for row, _ in planted}
        for row in {PASS, min(PASS + 255, n_sd - 1), n_sd - 1, n_sd - 2} - taken:
            planted.append((row, specs["precedence" if row % 2 else "two-cells"]))
    for cls in sorted(classes, key=lambda cls: specs[cls].axis != "h"):
        field.host(specs[cls], scale)  # (axis 0 first: its cells claim vertical faces as well)
    rows = []
    for row, spec in planted:
        cell = field.host(spec, scale)
        axis = 0 if spec.axis == "h" else dims - 1
        origin[:, row] = cell
        pos[axis, row] = spec.x
        if spec.axis == "h":
            pos[dims - 1, row] = 0.5
        j[row], mult[row] = spec.j, spec.n
        rows.append((row, spec.name))
    courant = tuple(field.faces)
    if scheme == IMPLICIT:  # it divides by 1 - (c_r - c_l) / n_substeps: never by zero
        for axis, component in enumerate(courant):
            for cell in np.argwhere(np.diff(component, axis=axis) == scale):
                face = tuple(cell + (np.arange(dims) == axis))
                assert not field.planted[axis][face], "planted faces that differ by 1"
                component[face] -= 1 / UNIT
            assert (np.diff(component, axis=axis) != scale).all()
    assert j.max() < J_MAX and mult.max() < 8 and n_sd < 2**20
    assert int((j * mult).sum()) < 2**53
    mass = j.astype(np.float64) * MASS_UNIT
    rtol = _substep_rtol(courant) if adaptive else 1e-2
    n_substeps = substeps_for(courant, rtol) if adaptive else 1
    assert n_substeps == scale
    perm, live = _compact(np.arange(n_sd, dtype=np.int64), mult, n_sd, n_sd)
    return Case(name=name, n_sd=n_sd, grid=grid, scheme=scheme, sed=sed, level=level,
                adaptive=adaptive, rtol=rtol, n_substeps=n_substeps,
                dt=DT_OVER_DZ * DZ * n_substeps, size=tuple(DZ * g for g in grid),
                courant=courant, origin=origin, pos=pos, mult=mult, mass=mass, classes=classes,
                cell_id=(origin * grid_strides(grid).reshape(-1, 1)).sum(axis=0),
                perm=perm, live=live, rows=tuple(rows), specs=specs, limit=limit, expected=[])


def _assert_planted(case, trace, after):  # pylint: disable=too-many-locals,too-many-branches
    """on the reference's intermediate values of the first step: every class present, every planted
    row where it was aimed, with the fate named in the module docstring"""
    first = trace[0]
    dims, top, level = len(case.grid), float(case.grid[-1]), float(case.level)
    position0 = np.full(case.n_sd + 1, -1)
    position0[case.perm[:case.live]] = np.arange(case.live)
    alive_after = np.zeros(case.n_sd, dtype=bool)
    alive_after[after["perm"][:after["live"]]] = True
    rained, left = set(first["rained"].tolist()), set(first["left"].tolist())
    by_class = {}
    for row, cls in case.rows:
        spec = case.specs[cls]
        axis = 0 if spec.axis == "h" else dims - 1
        by_class.setdefault(cls, []).append(row)
        landed, z = first["landed"][axis, row], first["z"][row]
        tag = f"{case.name}: row {row} of class {cls}"
        if spec.land is not None:
            assert bits(landed) == bits(spec.land), f"{tag} landed at {landed!r}"
        if spec.fate == "dead":
            assert position0[row] < 0 and case.mult[row] == 0 and case.mass[row] > 0, tag
            assert first["disp"][-1, row] < 0 and z < level, tag  # it would have been rain
            continue
        assert position0[row] >= 0, tag
        fate = "rain" if row in rained else "out" if row in left else "stay"
        assert fate == spec.fate, f"{tag}: {fate}, z = {z!r}"
        if spec.fate == "stay" and case.n_substeps == 1:
            assert alive_after[row], tag  # (and is compared)
        if cls == "top":
            assert z == top and after["origin"][-1, row] == 0, tag
        elif cls == "top+":
            assert z == np.nextafter(top, np.inf), tag
        elif cls == "level=":
            assert z == level and first["disp"][-1, row] < 0, tag
        elif cls == "level-":
            assert first["disp"][-1, row] < 0, tag
            assert z == np.nextafter(level, -np.inf) if level > 0 else -(2.0**-50) < z < 0, tag
        elif cls == "below,v=0":
            assert bits(first["disp"][-1, row]) == bits(0.0) and (z < level or level == 0), tag
        elif cls == "below,v=-0":
            assert bits(first["disp"][-1, row]) == bits(-0.0), tag
        elif cls == "below,v>0":
            assert first["disp"][-1, row] > 0 and (z < level or level == 0), tag
        elif cls == "precedence":
            assert z < 0 and first["disp"][-1, row] < 0 and case.mass[row] > 0, tag
        elif cls == "two-cells":
            assert first["disp"][-1, row] < -2 and z < level, tag
            assert case.origin[-1, row] >= level and case.mass[row] > 0, tag
        elif cls == "again":  # flagged in sub-step 1, and on the same course in sub-step 2
            second = trace[1]
            assert second["disp"][-1, row] < 0 and 0 <= second["z"][row] < level, tag
            assert row not in second["rained"].tolist() and case.mass[row] > 0, tag
        elif cls in ("zero+", "zero-", "carry1", "carry2"):
            assert bits(after["pos"][0, row]) == bits(-0.0 if cls == "zero-" else 0.0), tag
    for q, cls in enumerate(case.classes):
        rows = by_class.get(cls, [])
        want = 4 if case.n_sd >= FULL_FROM else min(4, len(range(q, case.limit, len(case.classes))))
        assert len(rows) >= want, f"{case.name}: class {cls} has {len(rows)} rows"
        if case.n_sd >= FULL_FROM and case.specs[cls].fate != "dead":
            waves = {int(position0[row]) // 64 for row in rows[:4]}
            assert len(waves) == 4, f"{case.name}: class {cls} in wavefronts {waves}"
    if case.sed:  # the fall range: more than a cell for the largest, far less for the smallest
        fallen = case.fall0 * DT_OVER_DZ
        if case.n_sd >= 63:
            assert fallen.max() > 1 and fallen[case.mass > 0].min() < 0.01, case.name
    if case.n_sd > PASS:  # the first pass of k_disp_precip alone would give another rainfall
        at, ids = first["rain_positions"], first["rained"]
        carried = np.abs(case.mass[ids]) * case.mult[ids]
        assert {PASS, min(PASS + 255, case.n_sd - 1), case.n_sd - 1} <= set(at.tolist())
        assert 0 < carried[at < PASS].sum() < carried.sum(), case.name


def expected_after(case, step, fall):
    """the reference's state after `step` calls (1-based), computed once per case and fall
    velocity and shared between the engines and routes"""
    cache = case.expected
    if step <= len(cache) and (fall is None or np.array_equal(cache[step - 1][0], fall)):
        return cache[step - 1][1]
    del cache[step - 1:]
    before = ({"perm": case.perm, "live": case.live, "origin": case.origin, "pos": case.pos}
              if step == 1 else cache[step - 2][1])
    trace = []
    after = reference_step(before, case, fall, trace)
    if step == 1:
        case.fall0 = fall
        _assert_planted(case, trace, after)
    cache.append((None if fall is None else fall.copy(), after))
    return after


def check_displacement(engine, name, route, steps=2):  # pylint: disable=too-many-locals
    case = make_case(name)
    pop = Population(engine, multiplicity=case.mult.copy(), mass=case.mass.copy(),
                     cell_id=case.cell_id.copy(), grid=case.grid,
                     cell_origin=case.origin.copy(), position_in_cell=case.pos.copy())
    runner = DisplacementRunner(pop, dt=case.dt, size=case.size, enable_sedimentation=case.sed,
                                precipitation_counting_level_index=case.level,
                                adaptive=case.adaptive, rtol=case.rtol, scheme=case.scheme,
                                route=route)
    runner.set_courant(case.courant)
    assert runner.n_substeps == case.n_substeps
    down = engine.download
    assert pop.live == case.live
    np.testing.assert_array_equal(down(pop.perm)[:pop.live], case.perm[:case.live])
    for step in range(1, steps + 1):
        fall = down(pop.fall_velocity(runner.law)) if case.sed else None
        rain = runner.run()
        want = expected_after(case, step, fall)
        tag = f"{name} {route} step {step}"
        assert pop.live == want["live"], f"{tag}: live {pop.live} != {want['live']}"
        ids = want["perm"][:want["live"]]
        np.testing.assert_array_equal(down(pop.perm)[:pop.live], ids, err_msg=tag + " perm")
        np.testing.assert_array_equal(down(pop.cell_origin)[:, ids], want["origin"][:, ids],
                                      err_msg=tag + " cell_origin")
        np.testing.assert_array_equal(down(pop.cell_id)[ids], want["cell_id"][ids],
                                      err_msg=tag + " cell_id")
        np.testing.assert_array_equal(down(pop.multiplicity)[ids], case.mult[ids],
                                      err_msg=tag + " multiplicity")
        np.testing.assert_array_equal(bits(down(pop.position_in_cell)[:, ids]),
                                      bits(want["pos"][:, ids]),
                                      err_msg=tag + " position_in_cell")
        assert rain == want["rain"], f"{tag}: rainfall {rain!r} != {want['rain']!r}"


# ---- the fall-velocity laws ---------------------------------------------------------------------
INTERPOLATION_LENGTHS = (255, 256, 257, 2**18 + 1)


def _either_side(values):
    values = np.asarray(values, dtype=np.float64)
    return np.concatenate([values, np.nextafter(values, np.inf), np.nextafter(values, -np.inf)])


@functools.lru_cache(maxsize=1)
def interpolation_radii():
    """every knot k * 1e-5 as computed in double, one ulp either side of it, 0, 6 mm exactly
    (which reads the last slope), one ulp below it, and r < 0 (the ice rows of a signed mass)"""
    knots = np.arange(601) * 1e-5
    radii = np.concatenate([[0.0, TABLE_TOP, -1e-6, -3e-3, np.nextafter(TABLE_TOP, 0)],
                            _either_side(knots)])
    radii = radii[radii <= TABLE_TOP]  # (one ulp above the table's top is outside the law)
    radii.setflags(write=False)
    return radii


def check_interpolation(engine, n):
    values, slopes = gunn_kinzer_table()
    factor = float(TABLE_POINTS_PER_METRE)
    radii = np.resize(interpolation_radii(), n)
    if n >= len(interpolation_radii()):
        radii = np.roll(radii, 101)  # (a knot at a workgroup's first and last thread)
    x = factor * radii
    i = np.where(radii < 0, 0, x).astype(np.int64)
    assert i.min() >= 0 and i.max() <= len(values) - 1
    if n >= len(interpolation_radii()):
        assert i.max() == len(values) - 1 and (radii < 0).any() and (np.fmod(x, 1.0) == 0).any()
    want = np.where(radii < 0, 0.0, values[i] + np.fmod(x, 1.0) / factor * slopes[i])
    out = engine.full(n, FLOAT, np.nan)
    engine.call("sdm_interpolation", out, engine.upload(radii), n, factor, engine.upload(values),
                engine.upload(slopes), len(values))
    np.testing.assert_array_equal(bits(engine.download(out)), bits(want),
                                  err_msg=f"interpolation {n}")


def check_rogers_yau(engine, n=257):
    law = RogersYau()
    small_k, medium_k, large_k, small_limit, medium_limit = law.consts
    radii = np.resize(np.concatenate([_either_side([small_limit, medium_limit]),
                                      [0.0, 1e-6, 2.5e-5, 1e-4, 5.9e-4, 1e-3, 5e-3]]), n)
    assert (radii == small_limit).any() and (radii == medium_limit).any()
    want = np.where(radii < small_limit, small_k * (radii * radii),
                    np.where(radii < medium_limit, medium_k * radii, large_k * np.sqrt(radii)))
    out = engine.full(n, FLOAT, np.nan)
    law.evaluate(engine, out, engine.upload(radii), n)
    np.testing.assert_array_equal(bits(engine.download(out)), bits(want), err_msg="Rogers-Yau")
