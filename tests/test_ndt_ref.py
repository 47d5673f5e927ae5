"""The CPU oracle's NDT voxel update against the exact single-voxel model (tests/ndt_ref.py) on the constructed states
and scripts of tests/ndt_cases.py.  The oracle was restated from the reference's code; the model from the equations.

Bars (every case, every event):
  * packed mean, count, is_miss and the NDT-TM hit / miss counts: exact;
  * value: within ONE float32 ulp, taken at max(|delta|, |initial|, |result|), of the unrounded exact value -- the
    float32 cast of the log-odds adjustment and the float32 sum round at most half such an ulp each, and the fp64 error
    of the likelihoods is orders of magnitude below that on these ranges;
  * factor terms: within one float32 ulp of the exact Cholesky term (half an ulp of storage rounding, the rest for the
    fp64 Gram-Schmidt update, whose error is the factor's condition number times 2^-53: at most 1e4 here).  One family,
    h_zero_diag, plants a SINGULAR factor (a zero diagonal): its condition number has no bound and the new third
    diagonal comes out of a cancellation, so it keeps the hit pin's 1e-6 relative (test_oracle_pins.py) instead;
  * intensity pair: 2 and 4 units of 2^-23 relative (ndt_cases.INTENSITY_BAR: counted float32 roundings).
A script is judged event by event, each transition from the state the oracle itself stored before it: the bars do not
compound, and a state the model merely propagated is never compared across a decision."""
import ctypes as C

import numpy as np
import pytest

import ndt_cases
import ndt_ref
from ndt_cases import Worst, geometry, judge, layers_of, make_oracle, oracle_tiles, plant, read_state, step_rays
from oracle.oracle import lib as olib

INF = float("inf")


@pytest.fixture(scope="module")
def built():
    return ndt_cases.build()


def test_every_cell_is_populated_and_clear_of_the_bands(built):
    sheets, stats = built
    assert set(stats) == set(ndt_cases.FAMILIES)
    for family, (config, per_cell, cells) in ndt_cases.FAMILIES.items():
        st = stats[family]
        for cell, _ in cells:
            assert st["cells"].get(cell, 0) == per_cell, (family, cell, st)
        assert st["band"] <= 0.01 * st["constructed"], (family, st)
    placed = sum(len(s.cases) for s in sheets)
    assert placed == sum(per_cell * len(cells) for _, per_cell, cells in ndt_cases.FAMILIES.values())
    for sheet in sheets:
        locals_ = [c.local for c in sheet.cases]
        assert len(set(locals_)) == len(locals_)


def test_every_ray_touches_exactly_its_own_target(built):
    sheets, _ = built
    for sheet in sheets:
        geo = geometry(sheet.config)
        for case in sheet.cases:
            for kind, sensor, sample, _ in case.events:
                assert geo.accepts(case.local, kind, sensor, sample), (case.family, case.cell, case.local)


def test_constructed_gaps_are_where_they_were_put(built):
    """Recomputed here from the stored fp64 rays: the decision sits on the wanted side of eta, at the wanted distance."""
    sheets, _ = built
    seen = set()
    for sheet in sheets:
        geo = geometry(sheet.config)
        for case in sheet.cases:
            if case.wanted_gap is None:
                continue
            step = ndt_ref.apply(geo.prm, case.state, case.model_events[0], geo.centre(case.local))
            name = {"m_gap": "prod", "h_tm_gap": "p_v" if case.cell[0] == "pv" else "prod_hit"}[case.family]
            got = float(step.gaps[name])
            g = abs(case.wanted_gap)
            assert got * case.wanted_gap > 0 and g / 2 <= abs(got) <= 2 * g, (case.family, case.cell, got)
            if case.family == "m_gap":
                assert step.is_miss == (case.wanted_gap < 0)
            else:
                before, after = case.state.hit_miss, step.state.hit_miss
                inc = (after[0] - before[0], after[1] - before[1])
                want = {("prod", True): (1, 0), ("prod", False): None, ("pv", True): (0, 1), ("pv", False): (0, 0)}[
                    (case.cell[0], case.wanted_gap > 0)]
                assert want is None or inc == want, (case.cell, inc)
                assert inc[0] == int(float(step.gaps["prod_hit"]) >= 0)
            seen.add((case.family, case.cell))
    assert len(seen) == 6 + 12


def test_families_reach_the_paths_they_are_named_for(built):
    """The state machine's edges are reached, by the model's own account of each case."""
    sheets, _ = built
    paths = {}
    for sheet in sheets:
        geo = geometry(sheet.config)
        for case in sheet.cases:
            steps = ndt_cases.run_model(geo.prm, case, geo.centre(case.local))
            paths.setdefault(case.family, []).append((case, steps))
    def all_(family, pred):
        assert all(pred(c, s) for c, s in paths[family]), family
    all_("m_unobserved", lambda c, s: s[0].path == "unobserved" and s[0].state.value == np.float32(geometry("A").prm.miss_value))
    all_("m_zero_diag", lambda c, s: s[0].path == "nan" and s[0].is_miss is False and s[0].state.value == c.state.value)
    all_("m_count_edge", lambda c, s: s[0].path == ("plain" if c.cell[0] < 0 else "ndt"))
    all_("m_through_mean", lambda c, s: s[0].state.value == np.float32(-2.0) and float(s[0].value_exact) == -2.0)
    all_("m_variance", lambda c, s: -15.96 < float(s[0].value_exact) - float(c.state.value) < -15.28)
    all_("m_prod0", lambda c, s: abs(float(s[0].value_exact) - float(c.state.value)) < 1e-12)
    all_("m_below_min", lambda c, s: s[0].state.value == np.float32(-2.0))
    all_("m_sat_min", lambda c, s: ("saturated" in s[0].path) == (c.cell[0] != "above"))
    all_("m_sat_max", lambda c, s: ("saturated" in s[0].path) == (c.cell[0] != "below"))
    all_("h_sat_max", lambda c, s: ("saturated" in s[0].path) == (c.cell[0] != "below"))
    all_("h_max", lambda c, s: "saturated" not in s[0].path and s[0].state.value == np.float32(3.511))
    all_("h_count0", lambda c, s: s[0].path == "init" and s[0].state.count == 1 and s[0].state.hit_miss == (1, 0))
    all_("h_reinit", lambda c, s: (s[0].path == "reinit") == (c.cell[0] >= 0 and "below" in c.cell[1]))
    all_("h_reinit_small_count", lambda c, s: (s[0].path == "reinit") == (c.cell[0] >= 0 and "below" in c.cell[1]))
    assert all(s[0].state.hit_miss == (1, 0) and s[0].state.count == 1 for c, s in paths["h_reinit"] if s[0].path == "reinit")
    all_("h_unobserved_counted", lambda c, s: s[0].state.hit_miss == (1, 0) and s[0].state.count == c.state.count + 1)
    all_("h_ak0", lambda c, s: s[0].state.cov == (0.0,) * 6)
    all_("s_reinit", lambda c, s: any(x.path == "reinit" for x in s) and any(x.path == "ndt" for x in s))
    all_("s_threshold", lambda c, s: {"plain", "ndt", "unobserved"} <= {x.path for x in s})
    for family, cases in paths.items():
        if family.startswith("s_"):
            assert all(6 <= len(c.events) <= 40 for c, _ in cases), family


def _leaf_transition(prm, case, centre):
    """One single-event case through the oracle's stand-alone leaves, chained the way the mapper chains them."""
    kind, sensor, sample, intensity = case.model_events[0]
    st = case.state
    mean = ndt_ref.voxel_mean(st.coord, centre, prm.resolution)
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])  # noqa: E731
    cov = (C.c_float * 6)(*st.cov)
    value = C.c_float(float(st.value))
    occ = C.c_float(float(st.value))
    if kind == "M":
        is_miss = C.c_int(-1)
        olib.oracle_calculate_miss_ndt(cov, C.byref(value), C.byref(is_miss), d3(sensor), d3(sample), d3(mean), st.count,
                                       INF, prm.miss_value, prm.adaptation_rate, prm.sensor_noise, prm.sample_threshold)
        olib.oracle_occupancy_adjust_down(C.byref(occ), float(st.value), value.value, INF, prm.min_value,
                                          float(prm.sat_min), float(prm.sat_max), 0)
        return np.float32(occ.value), tuple(cov), bool(is_miss.value), None
    reset = olib.oracle_calculate_hit_with_covariance(cov, C.byref(value), d3(sample), d3(mean), st.count, prm.hit_value,
                                                      INF, prm.resolution, prm.reinit_threshold, prm.reinit_count)
    olib.oracle_occupancy_adjust_up(C.byref(occ), float(st.value), value.value, INF, prm.max_value, float(prm.sat_min),
                                    float(prm.sat_max), 0)
    return np.float32(occ.value), tuple(float(v) for v in cov), None, bool(reset)


def test_oracle_leaves_hold_to_the_model(built, capsys):
    sheets, _ = built
    worst = Worst()
    for sheet in sheets:
        geo = geometry(sheet.config)
        for case in sheet.cases:
            if len(case.events) != 1:
                continue
            centre = geo.centre(case.local)
            value, cov, is_miss, reset = _leaf_transition(geo.prm, case, centre)
            step = ndt_ref.apply(geo.prm, case.state, case.model_events[0], centre)
            want = step.state
            if is_miss is not None:
                assert is_miss == step.is_miss, (case.family, case.cell, step.gaps)
            else:
                assert reset == (step.path.split("+")[0] in ("init", "reinit")), (case.family, case.cell)
            # the leaves do not touch mean, counters and intensity: judged on value and factor
            post = ndt_ref.State(value=value, cov=cov, coord=want.coord, count=want.count, intensity=want.intensity,
                                 hit_miss=want.hit_miss)
            worst.add(case.family, judge(geo.prm, case.state, case.model_events[0], centre, post, case.factor_bar))
    with capsys.disabled():
        worst.show("oracle leaves against the exact model (worst per family)")


def test_oracle_integrate_ndt_holds_to_the_model(built, capsys):
    sheets, _ = built
    worst = Worst()
    for sheet in sheets:
        geo = geometry(sheet.config)
        prm = geo.prm
        om = make_oracle(sheet.config)
        tiles = plant(om, sheet)
        whole = make_oracle(sheet.config)
        plant(whole, sheet)
        depth = max(len(c.events) for c in sheet.cases)
        for k in range(depth):
            cases, rays, intensities = step_rays(sheet, k)
            assert om.integrate_ndt(rays, intensities=intensities, flags=geo.flags) == len(cases)
            after = oracle_tiles(om, prm)
            for case in cases:
                vi = geo.index(case.local)
                out = judge(prm, read_state(tiles, vi), case.model_events[k], geo.centre(case.local),
                            read_state(after, vi), case.factor_bar)
                worst.add(case.family, out)
            tiles = after
        # the same events in one call: the mapper is sequential, so the same bits
        for rays, intensities in ndt_cases.all_rays(sheet):
            whole.integrate_ndt(rays, intensities=intensities, flags=geo.flags)
        final = oracle_tiles(whole, prm)
        for name in final:
            assert np.array_equal(final[name].view(np.uint32), tiles[name].view(np.uint32)), name
    with capsys.disabled():
        worst.show("oracle integrate_ndt against the exact model, event by event (worst per family)")
