"""CPU: the exact model of the voxel mean update (tests/mean_ref.py) against the oracle, on the constructed cases of
tests/mean_cases.py, and the conditions those cases have to meet for the GPU test (tests/test_gpu_mean_states.py) to
mean anything.

Measured here (seed 20240917): largest E 8.52e-13 of a cell, smallest margin of a forced axis 1.70e-13; 970 cases,
of the 580 tie cases 420 hold a near-tie and 579 sit within 2 ulp of a flip; 118 count-family axes have d == 0 exactly
and 8 cases reach NaN under the wrap that way.  The kill table is printed by
test_conditions_on_the_cases."""
import ctypes as C

import numpy as np
import pytest

import mean_cases
import mean_ref
from mean_cases import (COUNT_MUTANTS, CONFIGS, calls, check_case, geometry, make_oracle, oracle_integrate, plant,
                        read_voxel, sites_of, step_cases)
from oracle.oracle import lib as _olib


@pytest.fixture(scope="module")
def sheets():
    return mean_cases.build()


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def test_model_against_the_oracle_directly(sheets):
    """update_ref, the decode and the quantisation equal the oracle's three functions bit for bit on every sample of
    every case, from the model's own state before it."""
    samples = 0
    for sheet in sheets:
        geo = geometry(sheet.config)
        for case in sheet.cases:
            centre = geo.centre(case.local)
            coord, count = case.coord, case.count
            for end, state in zip(case.ends, case.states):
                v = [end[a] - centre[a] for a in range(3)]
                assert int(_olib.oracle_sub_voxel_update(coord, count, _d3(v), geo.res)) == state[0], (case, coord, count)
                local = (C.c_double * 3)()
                _olib.oracle_sub_voxel_to_local(coord, geo.res, local)
                assert tuple(local) == tuple(mean_ref.decode(c, geo.res) for c in mean_ref.cells_of(coord))
                assert int(_olib.oracle_sub_voxel_coord(_d3(v), geo.res)) == mean_ref.coord_ref(v, geo.res)
                assert int(_olib.oracle_sub_voxel_coord(local, geo.res)) == mean_ref.coord_ref(tuple(local), geo.res)
                coord, count = state
                samples += 1
    assert samples >= sum(len(sheet.cases) for sheet in sheets)


def test_model_against_the_oracle_through_the_mappers(sheets):
    """Planted sheets through OracleMap.integrate_occupancy (with and without kRfStopOnFirstOccupied) and integrate_ndt:
    every case's voxel after each of its rays is the model's, the count went up by one per ray (no ray was stopped or
    lost), forced axes hold floor(t_exact), and one call gives what one ray per voxel per call gives."""
    for sheet in sheets:
        geo = geometry(sheet.config)
        for site in sites_of(sheet.config):
            om = make_oracle(sheet, site)
            planted = plant(om, sheet, site)
            for name, tile in planted.items():
                assert np.array_equal(om.region_layer(geo.region, name).view(np.uint32), tile.view(np.uint32))
            for k, rays in enumerate(calls(sheet, lambda case, k: k)):
                oracle_integrate(om, site, rays)
                tiles = {"mean": om.region_layer(geo.region, "mean")}
                for case in step_cases(sheet, k):
                    got = read_voxel(tiles, geo, case)
                    assert got[1] == (case.count + k + 1) & 0xffffffff, (site, case.local, k, got)
                    check_case(case, k, got, "oracle, " + site)
            stepped = om.chunks()
            one = make_oracle(sheet, site)
            plant(one, sheet, site)
            (rays,) = calls(sheet)
            oracle_integrate(one, site, rays)
            for key, layers in one.chunks().items():
                for name, block in layers.items():
                    if name != "mean" and site == "ndt":
                        continue        # the covariance of a voxel depends on the mean its misses saw: not this test
                    assert np.array_equal(block.view(np.uint32), stepped[key][name].view(np.uint32)), (site, name)


def test_forced_cases_hold_the_exact_cell(sheets):
    """Where t_exact is further than E from an integer the model stores floor(t_exact) -- on every axis of every step."""
    forced = 0
    for sheet in sheets:
        for case in sheet.cases:
            for state, exact in zip(case.states, case.exact):
                for a, cell in enumerate(exact):
                    if cell is not None:
                        forced += 1
                        assert mean_ref.cells_of(state[0])[a] == cell, (case.family, case.config, case.local, a)
    assert forced > 1000


def kill_table(sheets, families=None):
    """(mutant, resolution, site) -> cases whose final state the mutant changes."""
    table = {}
    for sheet in sheets:
        res = CONFIGS[sheet.config][0]
        for site in sites_of(sheet.config):
            for case in sheet.cases:
                if families is None or case.family in families:
                    for m in case.kills:
                        table[(m, res, site)] = table.get((m, res, site), 0) + 1
    return table


def test_conditions_on_the_cases(sheets, capsys):
    cases = [c for sheet in sheets for c in sheet.cases]
    assert len(cases) == sum(sum(cfg[4]) for cfg in CONFIGS.values())           # every constructed case is here ...
    assert all(c.states is not None and len(c.states) == len(c.ends) == len(c.exact) for c in cases)   # ... and judged
    ties = [c for c in cases if c.family == "tie"]
    assert 4 * sum(c.near_tie or c.near_flip for c in ties) >= len(ties)
    sequences = [c for c in cases if c.family == "sequence"]
    assert all(2 <= len(c.ends) <= 6 and "order" in c.kills and c.near_flip for c in sequences)
    tiled = [s for s in sheets if s.config.startswith("tiled")]
    for sheet in tiled:       # cases in at least two of the z slabs the library cuts the region into
        dim = CONFIGS[sheet.config][1]
        assert dim // mean_cases.slab_layers(dim) >= 2
        assert len({c.local[2] // mean_cases.slab_layers(dim) for c in sheet.cases}) >= 2
    # the count family: every count edge on every planted style; samples tagged on_mean have d == 0 exactly, and at
    # least 4 cases per group of sites (the bar the count mutants have) reach 0 * inf = NaN under the wrap that way
    count_cases = [c for c in cases if c.family == "count"]
    assert {(c.count, c.tags[0]) for c in count_cases} == {(n, s) for n in mean_cases.COUNTS
                                                           for s in mean_cases.COUNT_STYLES}
    assert {kind for c in count_cases for kind in c.tags[1:]} >= set(mean_cases.SAMPLES)
    exact_axes = nan_cases = 0
    for c in count_cases:
        centre = geometry(c.config).centre(c.local)
        zero = [c.ends[0][a] - centre[a] == mean_ref.decode(mean_ref.cells_of(c.coord)[a], CONFIGS[c.config][0])
                for a in range(3)]
        for a in range(3):
            assert zero[a] == (c.tags[1 + a] == "on_mean") or c.tags[1 + a] not in ("on_mean", "near_mean"), c
        exact_axes += sum(zero)
        nan_cases += int(c.count == 0xffffffff and any(zero))
    assert exact_axes >= 16 and nan_cases >= 4, (exact_axes, nan_cases)
    every = kill_table(sheets)
    counts = kill_table(sheets, ("count",))
    with capsys.disabled():
        print("\nlargest E %.3e, smallest forced margin %.3e" % (max(c.bound for c in cases),
                                                                min(c.margin for c in cases)))
        print("count cases: axes with d == 0 exactly %d, cases with a NaN axis under the wrap %d" % (exact_axes,
                                                                                                  nan_cases))
        print("tie cases %d, with a near-tie %d, within 2 ulp of a flip %d" % (
            len(ties), sum(c.near_tie for c in ties), sum(c.near_flip for c in ties)))
        mean_cases.show_site_table(sheets)
        print("\ncases killed per (mutant, resolution, site); count family alone in brackets; '-' none")
        print("%-14s %5s %s" % ("mutant", "res", " ".join("%14s" % s for s in mean_cases.SITES)))
        for m in mean_ref.MUTANTS:
            for res in (0.1, 0.25):
                cells = []
                for site in mean_cases.SITES:
                    n, nc = every.get((m, res, site), 0), counts.get((m, res, site), 0)
                    cells.append("%14s" % (("%d (%d)" % (n, nc)) if n else "-"))
                print("%-14s %5s %s" % (m, res, " ".join(cells)))
        print("closed_centre is empty at 0.25 where the map origin is 0: every term of both forms is exact there;\n"
              "recip_grid is empty at 0.1, as in the probe that motivated these tests; the tiled site holds the tie\n"
              "family only, so `order` and the count mutants have no cases there.")
    for site in mean_cases.SITES:
        both = lambda m, table=every: table.get((m, 0.1, site), 0) + table.get((m, 0.25, site), 0)  # noqa: E731
        for m in ("fma", "div_count", "closed_centre"):
            assert both(m) >= 16, (m, site, both(m))
        assert every.get(("recip_grid", 0.25, site), 0) >= 16, site
        if site == "tiled":
            continue                      # tie family only
        assert both("order") >= 16, site
        for m in COUNT_MUTANTS:
            assert both(m, counts) >= 4, (m, site, both(m, counts))
