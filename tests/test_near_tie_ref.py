"""The near-tie rays of tests/near_tie_cases.py, without a GPU: the generator's own coverage and bookkeeping, and the CPU
oracle against the exact walker on every kept ray.

The second part is what the GPU tests (tests/test_gpu_near_tie.py) stand on: the device is held bit-identical to the
oracle, the oracle's fp64 walk is shown here to decide every one of these gaps -- down to 2e-8 of a step and 0.02 of the
predictor's margin -- as exact arithmetic does, so on these rays "identical to the CPU" and "right" are one demand.

Not here: the same comparison through oracle/_ref.  The reference's ohm/LineWalkCompute.h needs glm, which the recipe
in oracle/Makefile deliberately does not stand in for, so the shim exports no line walk to compare with."""
import collections
from fractions import Fraction
from math import isqrt

import pytest

import near_tie_cases as N
from exact_walk import walk

FAMILIES = ("A", "B", "C")
CONFIG_NAMES = tuple(N.CONFIGS)
WALK_EXCLUDE_START, WALK_EXCLUDE_END = 1, 2     # oracle/ohm_oracle.h: what kRfExcludeOrigin / the default sample rule ask of the walk


@pytest.mark.parametrize("cfg", CONFIG_NAMES)
def test_every_cell_is_populated_and_discarding_is_capped(cfg):
    for family in FAMILIES:
        kept, discarded = N.generate(family, cfg)
        thrown = sum(discarded.values())
        assert thrown <= (len(kept) + thrown) // 2, (family, cfg, discarded)
        assert len(kept) >= (500 if family != "C" else 400), (family, cfg, len(kept), discarded)
        assert len({c["start"] + c["end"] for c in kept}) == len(kept)
    tile = N.CONFIGS[cfg]["tile"]
    # family A: every gap, either axis first, at every position
    kept, _ = N.generate("A", cfg)
    cells = collections.Counter((c["gap_cell"], c["first_cell"], p) for c in kept for p in c["positions"])
    empty = [(str(g), f, p) for g in N.GAPS_A for f in "ab" for p in N.POSITIONS_A if not cells[(g, f, p)]]
    assert not empty, empty
    for c in kept:
        a, b = c["axes"]
        if "late" in c["positions"]:
            assert c["steps_in_tile"][a] >= tile[a] - 2 and c["steps_in_tile"][b] >= tile[b] - 2
        if "early" in c["positions"]:
            assert sum(c["steps_in_tile"]) <= 1
        assert abs(c["gap_margins"] - c["gap_cell"]) <= Fraction(1, 100)
        assert (c["gap_margins"] > 1) == (c["gap_cell"] > 1)
    # family B: every gap, either axis first, at the 1st, 2nd and a 5th or later tile entry
    kept_b, _ = N.generate("B", cfg)
    cells = collections.Counter((c["gap_cell"], c["first_cell"], c["entry"]) for c in kept_b)
    empty = [(str(g), f, e) for g in N.GAPS_B for f in "ab" for e in N.ENTRIES_B if not cells[(g, f, e)]]
    assert not empty, empty
    for c in kept_b:
        assert abs(c["gap_steps_b"] / c["gap_cell"] - 1) <= Fraction(1, 20)
        assert (c["gap_steps_b"] > N.BAND_STEPS) == (c["gap_cell"] > N.BAND_STEPS)
    assert {c["xclass"] for c in kept_b} >= {"neg", "unit", "large"}
    assert {c["wall"] for c in kept_b} >= {"exit", "opposite"}
    for family, cases in (("A", kept), ("B", kept_b)):
        assert {frozenset(c["axes"]) for c in cases} == {frozenset(p) for p in ((0, 1), (0, 2), (1, 2))}
        assert {c["signs"] for c in cases if c["third"] != "idle"} == set(N.SIGNS), family
        assert {c["third"] for c in cases} >= {"idle", "active", "exhausted_in_segment"}, family
    # family C: exact (structural) ties at the same positions and entries
    kept_c, _ = N.generate("C", cfg)
    assert all(c["tie"] and c["gap_u"] == 0 for c in kept_c)
    positions = set().union(*(c["positions"] for c in kept_c))
    assert positions >= {"early", "first", "third+"}
    if len(set(tile)) < 3:      # a late tie needs two axes with the same tile edge
        assert "late" in positions
    assert {c["entry"] for c in kept_c} >= {"1", "2", "5+"}


@pytest.mark.parametrize("cfg", CONFIG_NAMES)
def test_recorded_gap_is_the_gap_of_the_recorded_comparison(cfg):
    """Recomputed here from the end points and the two step indices alone: step k of an axis is taken at ray parameter
    (x + (k - 1) voxel) / |d|, x the distance from the start to its voxel's wall in the direction of travel."""
    config = N.CONFIGS[cfg]
    tile, origin = config["tile"], config["origin"]
    diagonal_m = Fraction(isqrt(sum(t * t for t in tile) << 100), 1 << 50) / 8
    unit_m = Fraction(101, 100) * diagonal_m / 2 ** 30          # ohmhip_map.hip:136-141
    margin = 2 * max(tile) + 8
    for family in FAMILIES:
        kept, _ = N.generate(family, cfg)
        for c in kept:
            s, e = c["start_units"], c["end_units"]
            u = {}
            for axis, k in zip(c["axes"], c["step_index"]):
                d = e[axis] - s[axis]
                inside = (s[axis] - origin[axis]) % N.SUB
                x = inside if d < 0 else N.SUB - inside
                u[axis] = Fraction(x + (k - 1) * N.SUB, abs(d))
            a, b = c["axes"]
            assert abs(u[a] - u[b]) == c["gap_u"]
            if not c["tie"]:
                assert u[c["first_axis"]] < u[c["other_axis"]]
                assert c["gap_u"] > Fraction(1, 10 ** 9) * max(u.values())      # the exact walker's contract
            length_m = Fraction(isqrt(sum((q - p) ** 2 for p, q in zip(s, e)) << 100), 1 << 50) / 2 ** 33
            assert abs(c["gap_m"] / (c["gap_u"] * length_m) - 1) < 1e-11 if c["gap_u"] else c["gap_m"] == 0
            assert abs(c["gap_units"] * unit_m - c["gap_m"]) <= c["gap_m"] * Fraction(1, 10 ** 11)
            assert c["gap_margins"] * margin == c["gap_units"]
            if c["other_gap_m"] is not None:
                assert c["other_gap_m"] >= N.ISOLATION * margin * unit_m * (1 - Fraction(1, 10 ** 9))
            assert tuple(float(v) * 2.0 ** 33 for v in c["start"] + c["end"]) == tuple(float(v) for v in s + e)
            assert max(abs(v) for v in s + e) < 2 ** 40
            assert len({k[0] for k in c["keys"]}) <= N.MAX_REGIONS


@pytest.mark.parametrize("cfg", CONFIG_NAMES)
def test_kept_rays_are_inside_the_exact_walkers_contract(cfg):
    """walk() raises Undecidable for a comparison closer than 1e-9 relative that is no structural tie: never on a kept
    ray, and the sequence it gives is the recorded one."""
    config = N.CONFIGS[cfg]
    for family in FAMILIES:
        kept, _ = N.generate(family, cfg)
        for c in kept:
            keys = walk(c["start_units"], c["end_units"], sub=N.SUB, region=config["region"],
                        origin_units=config["origin"])
            assert keys == c["keys"]


@pytest.mark.parametrize("cfg", CONFIG_NAMES)
def test_oracle_walk_equals_the_exact_walker_on_near_ties(cfg):
    from oracle.oracle import OracleMap
    config = N.CONFIGS[cfg]
    om = OracleMap(N.RES, config["region"])
    om.set_origin(N.to_metres(config["origin"]))
    for family in FAMILIES:
        kept, _ = N.generate(family, cfg)
        for i, c in enumerate(kept):
            keys = c["keys"]
            assert len(keys) >= 2
            for flags, expect in ((0, keys),                                # kRfEndPointAsFree: the end voxel is walked
                                  (WALK_EXCLUDE_END, keys[:-1]),            # default flags
                                  (WALK_EXCLUDE_START, keys[1:]),           # kRfExcludeOrigin | kRfEndPointAsFree
                                  (WALK_EXCLUDE_START | WALK_EXCLUDE_END, keys[1:-1])):     # kRfExcludeOrigin
                got, _, _ = om.walk(c["start"], c["end"], flags, cap=1024)
                assert got == expect, (family, cfg, i, flags, c["start"], c["end"], str(c["gap_cell"]), c["positions"],
                                       c["entry"], float(c["gap_units"]))
