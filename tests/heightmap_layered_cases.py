"""Scenes of the layered heightmap tests (CPU restatement and device) -- TEST INFRASTRUCTURE.  Built on the flood fill's
scenes (tests/heightmap_fill_cases.py: Scene, the multi-level scene, the mean scene).

staircase()       hand-made: six steps of three columns, each a voxel higher than the last
two_storey()      hand-made: a ground floor of 12 x 12 columns over four 8^3 regions, an upper floor over part of it
                  that reaches two map corners, a ramp between them, and columns without a floor voxel ("holes": a
                  virtual surface, or nothing) at chosen places.  Every column of interest lies on or beside the region
                  boundary at x = 0 / y = 0.
HAND_MADE         (id, scene arguments, Params arguments, mode, threshold, the quirks the case exists for): each quirk
                  is a count of tests/heightmap_layered_ref.py's `quirks` or of its stats that must be > 0
layered_cases()   every (id, Scene, Params, mode, threshold, quirks) the two formulations are compared on"""
from heightmap_ref import Params
from heightmap_fill_cases import HIT, MISS, Scene, mean_scene, scaled_multi_level

MODE_UNORDERED, MODE_ORDERED = 2, 3

FLOOR, TOP = 1, 5       # global z of the two storeys
LO, HI = -6, 6          # columns x, y in [LO, HI)
TOP_X = -2              # the upper floor covers x >= TOP_X
RAMP_Y = (-1, 0)        # the ramp's two rows, either side of the region boundary
#: columns without a floor voxel: in the open by the ramp, alone in the open, at a map corner in the open, at a map
#: corner under the upper floor, and under the upper floor's middle
HOLE_BY_RAMP, HOLE_OPEN, HOLE_CORNER, HOLE_TOP_CORNER, HOLE_UNDER = (-5, 1), (-4, -4), (-6, -6), (5, 5), (1, 0)
HOLES = (HOLE_BY_RAMP, HOLE_OPEN, HOLE_CORNER, HOLE_TOP_CORNER, HOLE_UNDER)


def two_storey(observed_top=True, mean=False):
    """The upper floor's voxels have a free voxel above them only with observed_top: without it they are no base-layer
    candidates (no clearance, nothing observed above)."""
    s = Scene(1.0, (8, 8, 8), mean)
    for y in range(LO, HI):
        for x in range(LO, HI):
            if (x, y) not in HOLES:
                s.put((x, y, FLOOR), HIT)
            s.put((x, y, FLOOR + 1), MISS)
            if x >= TOP_X:
                s.put((x, y, TOP), HIT)
                if observed_top:
                    s.put((x, y, TOP + 1), MISS)
    for y in RAMP_Y:
        for x in range(LO, TOP_X):  # z = FLOOR + 1 .. TOP: the last step is level with the upper floor
            z = FLOOR + 1 + (x - LO)
            s.put((x, y, z), HIT)
            s.put((x, y, z + 1), MISS)
    return s


def staircase(steps=6):
    """Steps of 3 columns each, one voxel higher per column of x, with a free voxel above each; they straddle the region
    boundaries at x = 0 and y = 0."""
    s = Scene(1.0, (8, 8, 8), False)
    for i in range(steps):
        for y in (-1, 0, 1):
            s.put((i - 3, y, FLOOR + i), HIT)
            s.put((i - 3, y, FLOOR + i + 1), MISS)
    return s


def _params(seed_level=FLOOR, **kw):
    """The seed over column (-5, 4) at the height of the centre of global voxel z = seed_level (region 0 spans -4 .. 4)."""
    return dict(dict(grid_resolution=1.0, min_clearance=0.0, reference_pos=(-8.5, 0.5, seed_level - 3.5)), **kw)


#: id, two_storey() arguments, Params arguments, mode, filter threshold, quirks
HAND_MADE = (
    ("repeat-and-seed-again", {}, _params(), MODE_ORDERED, 0, ("repeats", "multi_layer_columns", "seed_column_again")),
    ("column-rule", {}, _params(), MODE_ORDERED, 0, ("column_rule_refusals",)),
    ("too-close-real", {}, _params(grid_resolution=2.0, min_clearance=1.0), MODE_ORDERED, 0,
     ("too_close", "too_close_real")),
    ("sort-permutes", {}, _params(), MODE_ORDERED, 0, ("permuted_columns",)),
    ("base-by-clearance", {"observed_top": False}, _params(seed_level=TOP), MODE_ORDERED, 0, ("base_not_nearest",)),
    ("base-by-distance", {}, _params(seed_level=TOP), MODE_ORDERED, 0, ("base_by_distance",)),
    ("base-tie", {}, _params(seed_level=0.5 * (FLOOR + TOP)), MODE_ORDERED, 0, ("base_ties",)),
    ("filter-single-and-multi", {}, _params(virtual_surface=True, ceiling=2.0), MODE_ORDERED, 4,
     ("filtered", "filtered_single", "filtered_multi", "virtual_kept")),
    ("unordered-two-base", {}, _params(), MODE_UNORDERED, 0, ("two_base_columns",)),
    ("mean-coarse", {"mean": True}, _params(grid_resolution=2.0, origin=(0.5, 0.5, 0.0)), MODE_ORDERED, 0,
     ("multi_layer_columns", "mean_in_upper_slot")),
)


def hand_made_cases():
    for name, scene_kw, params_kw, mode, threshold, quirks in HAND_MADE:
        yield name, two_storey(**scene_kw), Params(**params_kw), mode, threshold, quirks
    # one heightmap cell over the whole staircase: a column of six voxels, a step per generation; generation 1 alone
    # makes five adds to it (plane_growth())
    stairs = staircase()
    yield ("six-storeys", stairs, Params(6.0, 0.0, reference_pos=stairs.centre((-3, 0, FLOOR)), origin=(5.0, 5.0, 0.0)),
           MODE_ORDERED, 0, ("multi_layer_columns", "repeats"))
    # every up axis: the scene turned, the seed with it
    base = two_storey()
    kw = _params(virtual_surface=True, ceiling=2.0)
    for up_axis in (-3, -2, -1, 0, 1):
        turned = dict(kw, up_axis=up_axis, reference_pos=base.point_permuted(kw["reference_pos"], up_axis))
        yield "up%d" % up_axis, base.permuted(up_axis), Params(**turned), MODE_ORDERED, 4, ("filtered", "permuted_columns")


def quirk_counts(res):
    """Every count a case may name: the restatement's stats and quirks, and what is read off its arrays."""
    import heightmap_layered_ref as LR
    counts = dict(zip(LR.STATS, LR.stats_of(res)))
    counts.update(res.quirks)
    seed = tuple(res.log[0][:2].tolist())
    counts["seed_column_again"] = sum(tuple(v[:2]) == seed for v in res.log[1:].tolist())
    in_use = res.occupancy != float("inf")
    counts["two_base_columns"] = int(((in_use & (res.voxels["layer"] == LR.HVL_BASE)).sum(axis=0) >= 2).sum())
    counts["virtual_kept"] = int((res.occupancy == -1.0).sum())
    counts["mean_in_upper_slot"] = int((res.mean[1:, :, :, 1] != 0).sum()) if res.mean is not None else 0
    return counts


def plane_growth(res, initial=2):
    """How the device's slot planes must grow on this walk: [(capacity before, slots asked for)] for every generation
    after which they do.  A heightmap cell asks for the voxels its column held before the generation plus every add the
    generation makes to it, stood or not; the planes start at `initial` slots and grow to max(asked, 2 * capacity)."""
    ends = []
    for size in res.generation_sizes:
        ends.append(size + (ends[-1] if ends else 0))
    asked = [{} for _ in ends]
    generation = 0
    for visit, cell, held in res.add_trace:  # in visit order
        while visit >= ends[generation]:
            generation += 1
        asked[generation][cell] = asked[generation].get(cell, held) + 1
    capacity, grown = initial, []
    for cells in asked:
        most = max(cells.values(), default=0)
        if most > capacity:
            grown.append((capacity, most))
            capacity = max(most, 2 * capacity)
    return grown


def layered_cases():
    """(id, Scene, Params, mode, threshold, quirks) of every case."""
    for case in hand_made_cases():
        yield case
    for up_axis in (-3, -2, -1, 0, 1, 2):
        scene, p = scaled_multi_level(up_axis)
        for mode in (MODE_UNORDERED, MODE_ORDERED):
            for threshold in (0, 8):
                quirks = ("repeats",) + (("multi_layer_columns",) if mode == MODE_ORDERED else ()) + \
                    (("filtered", "virtual_kept") if mode == MODE_ORDERED and threshold else ())
                yield "multi-level-up%d-mode%d-t%d" % (up_axis, mode, threshold), scene, p, mode, threshold, quirks
    scene = mean_scene()
    yield ("mean-same", scene, Params(0.5, 0.0, reference_pos=(0.1, 0.1, 0.0), origin=(0.25, 0.25, 0.0), region_size=16),
           MODE_ORDERED, 0, ())
