"""CPU: the occupancy log-odds model (tests/occupancy_ref.py) and its sheets (tests/occupancy_cases.py).

  * every operation of the model on a grid of edge states x flag subsets x saturation settings x null_update equals the
    same expression in exact rational arithmetic rounded once, the oracle's oracle_occupancy_adjust_* entry points and,
    where oracle/_ref is built, the reference header itself;
  * the model equals the CPU oracle bit for bit on every sheet after every call;
  * every listed edge state, flag subset, pattern and count edge is reached on every site it applies to -- counted from
    the model's own event lists;
  * the sheets of every site meet the conditions that select that site's path on the device (batch_run.h,
    walk_kernel.h): the device exposes no path counters, so construction is the evidence;
  * every mutant of the model changes at least one voxel of at least one sheet on every site it applies to (APPLIES)."""
import ctypes as C
import os

import numpy as np
import pytest

import occupancy_cases as OC
import occupancy_ref as O
from occupancy_ref import F
from oracle import oracle as orc
from traversal_ref import RF_END_POINT_AS_FREE, RF_EXCLUDE_ORIGIN, RF_STOP_ON_FIRST_OCCUPIED

_OP = tuple(m for m in O.OP_MUTANTS if m != "null_update_adjusts")
_RUN = ("n_misses_as_one_product", "misses_all_before_hits", "trailing_misses_dropped")
# Which mutant the sheets of which site must tell from the model.  Not listed: null_update_adjusts and the three stop
# mutants off the stop site (no other site has null updates or stops); the run mutants ON the stop site (its replay has
# no runs to count); count_mod_2_15 / 2_16 off maxchunk (no other site sends 2^15 rays through a voxel);
# config_of_previous_call where no sheet changes its configuration; threshold_strict and classify_after_update where no
# sheet sets a value-exclusion flag or stops; on maxchunk everything that needs another state than 1.0 under tiny
# misses; sat_closed and classify_after_update on stop (the default configuration does not saturate, and the stop
# decision is made before the miss by construction).
APPLIES = {
    "walk": _OP + _RUN + ("config_of_previous_call",),
    "lists": _OP + _RUN + ("config_of_previous_call",),
    "dense": ("sat_closed", "unobserved_keeps_inf_base", "clamp_then_add", "nan_propagates", "zero_sign_kept") + _RUN,
    "mean": _OP + _RUN,
    "odd": _OP + _RUN,
    "half": _OP + _RUN,
    "tiled": _OP + _RUN,
    "spill": ("sat_closed", "unobserved_keeps_inf_base", "clamp_then_add", "nan_propagates", "zero_sign_kept") + _RUN,
    "stop": ("threshold_strict", "unobserved_keeps_inf_base", "clamp_then_add", "nan_propagates", "zero_sign_kept",
             "null_update_adjusts") + O.STOP_MUTANTS,
    "maxchunk": ("n_misses_as_one_product", "misses_all_before_hits", "count_mod_2_15", "count_mod_2_16"),
}
STATES_SITES = ("walk", "lists", "dense", "mean", "odd", "half", "tiled", "spill")     # every state x every pattern
FLAGS_SITES = ("walk", "lists", "mean", "odd", "half", "tiled")                        # every subset x every pattern
COUNT_EDGES = {"walk": (OC.N,), "lists": (OC.N + 1,), "mean": (OC.N, OC.N + 1), "half": (OC.N, OC.N + 1),
               "maxchunk": (OC.MAX_CHUNK, OC.MAX_CHUNK + 1, (1 << 15) + 1, (1 << 16) + 1)}


@pytest.fixture(scope="module")
def sheets():
    return {site: OC.build(site) for site in OC.SITES}


def same(a, b):
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return bool(a.view(np.uint32) == b.view(np.uint32)) or bool(np.isnan(a) and np.isnan(b))


def grid():
    """(cfg, state name, x, flags, hit, null_update) over the edge states of six configurations x the four saturation
    settings x every flag subset."""
    for name in ("default", "clamp0", "miss_half", "pos_threshold", "tiny", "tight_00"):
        base = OC.configs()[name]
        for sat_min in (False, True):
            for sat_max in (False, True):
                cfg = base._replace(sat_min=sat_min, sat_max=sat_max)
                for state, x in OC.edge_states(cfg).items():
                    for flags in O.VALUE_FLAG_SUBSETS:
                        for hit in (False, True):
                            for null in (False, True):
                                yield cfg, state, x, flags, hit, null


def through(lib, prefix, cfg, x, flags, hit, null):
    """occupancyAdjustHit / Miss of a C library, handed the adjustment the mapper's selects leave."""
    fn = getattr(lib, prefix + ("hit" if hit else "miss"))
    lo, hi = O.window(cfg)
    out = C.c_float(float(x))
    fn(C.byref(out), float(x), float(O.selected(cfg, x, flags, hit)), float("inf"),
       float(cfg.max_value if hit else cfg.min_value), float(lo), float(hi), int(null))
    return F(out.value)


def test_every_operation_against_exact_arithmetic_and_the_oracle():
    n = 0
    for cfg, state, x, flags, hit, null in grid():
        got = O.adjust(cfg, x, flags, hit, null)
        what = (cfg, state, flags, hit, null, got)
        assert same(got, O.adjust_exact(cfg, x, flags, hit, null)), what
        assert same(got, through(orc.lib, "oracle_occupancy_adjust_", cfg, x, flags, hit, null)), what
        n += 1
    assert n > 20000
    # what the rule's docstring says of the edges
    cfg = OC.configs()["clamp0"]
    assert O.bits(O.adjust_miss(cfg, F(-0.0))) == O.bits(F(0.0))                  # -0.0 + 0.0 is +0.0, and is stored
    assert O.bits(O.adjust_miss(OC.configs()["default"], F(-0.0), O.RF_EXCLUDE_OCCUPIED)) == O.bits(F(0.0))
    assert O.adjust_miss(cfg, OC.NAN) == cfg.min_value and O.adjust_hit(cfg, OC.NAN) == cfg.max_value
    assert O.adjust_miss(OC.configs()["default"], F(-7.0), 0, True) == F(-2.0)    # a null update still clamps
    assert O.adjust_miss(OC.configs()["default"], O.FLT_MAX) == O.FLT_MAX         # x < sat_max freezes FLT_MAX


def test_every_operation_against_the_reference_header():
    if not os.path.exists(orc.REF_LIB_PATH):
        pytest.skip("oracle/_ref/libohmref.so not built (reference checkout absent)")
    ref = C.CDLL(orc.REF_LIB_PATH)
    for n in ("hit", "miss"):
        getattr(ref, "ref_occupancy_adjust_" + n).argtypes = [C.POINTER(C.c_float)] + [C.c_float] * 6 + [C.c_int]
    for cfg, state, x, flags, hit, null in grid():
        got = O.adjust(cfg, x, flags, hit, null)
        theirs = through(ref, "ref_occupancy_adjust_", cfg, x, flags, hit, null)
        assert same(got, theirs), (cfg, state, flags, hit, null)


def test_landing_and_overshooting_states_do_what_their_names_say():
    for name, cfg in OC.configs().items():
        if cfg.miss == 0 or F(cfg.min_value - cfg.miss) == cfg.min_value:
            continue                            # (no miss moves anything there: nothing lands, nothing overshoots)
        states = OC.edge_states(cfg)
        free = cfg._replace(sat_min=False, sat_max=False)
        for k in (1, 2, 3):
            assert "land%d" % k in states, (name, k)
            x = states["land%d" % k]
            for i in range(k):
                assert x > cfg.min_value
                x = F(x + cfg.miss)                                 # unclamped: the k-th add lands exactly on min
            assert x == cfg.min_value, (name, k)
            x = states["over%d" % k]
            for i in range(k - 1):
                x = O.adjust_miss(free, x)
                assert x > cfg.min_value, (name, k)
            assert F(x + cfg.miss) < cfg.min_value and O.adjust_miss(free, x) == cfg.min_value, (name, k)
    tiny = OC.configs()["tiny"]
    stuck = OC.edge_states(tiny)["stuck"]
    assert tiny.min_value < stuck and F(stuck + tiny.miss) == stuck    # x + miss == x under wide clamps


def test_the_model_equals_the_oracle_on_every_sheet(sheets):
    seen = set()
    for site in OC.SITES:
        for sheet in sheets[site]:
            if sheet.name in seen:
                continue
            seen.add(sheet.name)
            unknown = np.full(sheet.mp.volume, np.inf, dtype=F)
            om = OC.make_oracle(sheet)
            for k, call in enumerate(sheet.calls):
                OC.set_oracle_config(om, call.cfg)
                om.integrate_occupancy(call.rays, flags=call.flags)
                theirs = om.chunks(["occupancy"])
                for region in set(theirs) | set(sheet.states[k]):
                    a = theirs[region]["occupancy"] if region in theirs else unknown
                    b = sheet.states[k].get(region, unknown)
                    d = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
                    assert not len(d), (sheet.name, k, region, sheet.mp.local(int(d[0])), a[d[0]], b[d[0]])


def reached(sheet):
    """{(state, pattern, flags)} of the cells whose target voxel got exactly the cell's pattern in the cell's call."""
    out = set()
    patterns = [O.patterns_of(e) for e in sheet.events]
    for cell in sheet.cells:
        if patterns[cell.call].get(cell.target, "") == cell.pattern:
            out.add((cell.state, cell.pattern, cell.flags))
    return out


def test_every_state_flag_subset_pattern_and_count_edge_is_reached(sheets):
    for site in OC.SITES:
        got = set()
        for sheet in sheets[site]:
            got |= {(sheet.name.split("/")[0], sheet.name.split("/")[1]) + r for r in reached(sheet)}
        if site in STATES_SITES:
            for cfg_name in {g[1] for g in got if g[0] in ("states", "dense")}:
                for state in OC.edge_states(OC.configs()[cfg_name]):
                    for pattern in OC.PATTERNS:
                        want = (cfg_name, state, pattern, 0)
                        assert any(g[1:] == want for g in got), (site,) + want
            assert any(g[0] in ("states", "dense") for g in got), site
        if site in FLAGS_SITES:
            for subset in O.VALUE_FLAG_SUBSETS:
                for state in OC.FLAG_STATES:
                    for pattern in OC.PATTERNS:
                        assert any(g[0] == "flags" and g[2:] == (state, pattern, subset) for g in got), (
                            site, subset, state, pattern)
        for n in COUNT_EDGES.get(site, ()):
            assert any(g[0] == "count" and g[2:4] == ("count%d" % n, "m" * n) for g in got), (site, n)
            if n <= OC.MAX_CHUNK + 1:
                assert any(g[0] == "count" and g[2:4] == ("count%d" % n, "h" + "m" * (n - 1)) for g in got), (site, n)
    # the states that only matter under one configuration are there under it
    walk = {r for s in sheets["walk"] if s.name.startswith("states/") for r in
            [(s.name.split("/")[1],) + c for c in reached(s)]}
    assert ("tiny", "stuck", "mmm", 0) in walk and ("tight_00", "flt_max", "m", 0) in walk
    assert ("clamp0", "-0", "m", 0) in walk and ("miss_half", "-0", "m", 0) in walk


def test_the_stop_sheets_stop_where_they_are_built_to(sheets):
    for sheet in sheets["stop"]:
        flags = sheet.calls[0].flags
        assert all(c.flags & RF_STOP_ON_FIRST_OCCUPIED for c in sheet.calls)
        events = sheet.events[0]
        sampled = {e.ray for e in events if e.kind == "h"}
        nulls = [e for e in events if e.kind == "n"]
        first, n = sheet.chain
        if not flags & RF_END_POINT_AS_FREE:
            # the staircase: ray i stops exactly if ray i - 1 did not
            stopped = [first + i not in sampled for i in range(n)]
            assert n >= 40 and stopped[0] is False
            assert all(stopped[i] != stopped[i - 1] for i in range(1, n)), stopped
        if not flags & RF_EXCLUDE_ORIGIN:
            assert nulls                                   # (every ray of these rows starts next to its wall otherwise)
        tile, mp = sheet.planted[(0, 0, 0)], sheet.mp
        states = OC.edge_states(sheet.calls[0].cfg)
        names = list(states)
        # a wall at the threshold stops its ray (the voxel behind it gets a null update); one ulp below does not
        behind = {(e.key[1], e.kind) for e in events if e.ray < 2 * len(names)}
        for name, stops in (("thr", True), ("thr-", False), ("nan", False), ("inf", False), ("max", True)):
            ly = names.index(name)
            assert tile[mp.index((12, ly, 2))].view(np.uint32) == states[name].view(np.uint32)
            assert ((mp.index((13, ly, 2)), "n") in behind) == stops, name
        # null updates meet values that they change: a NaN, a -0.0, a value below min
        hit_by_null = {tile[e.key[1]].view(np.uint32).item() for e in nulls if e.key[0] == (0, 0, 0)}
        for name in ("nan", "-0", "below_min", "-inf"):
            assert states[name].view(np.uint32).item() in hit_by_null, name
    assert {s.calls[0].flags & (RF_END_POINT_AS_FREE | RF_EXCLUDE_ORIGIN) for s in sheets["stop"]} == {
        0, RF_END_POINT_AS_FREE, RF_EXCLUDE_ORIGIN}


def test_the_sheets_of_every_site_meet_the_conditions_of_its_path(sheets):
    for site in OC.SITES:
        for sheet in sheets[site]:
            volume = sheet.mp.volume
            stop = any(c.flags & RF_STOP_ON_FIRST_OCCUPIED for c in sheet.calls)
            assert stop == (site == "stop"), sheet.name
            segments = [sheet.segments(k) for k in range(len(sheet.calls))]
            samples = [sheet.samples(k) for k in range(len(sheet.calls))]
            most_samples = max(max(s.values(), default=0) for s in samples)
            lds_hits = OC.LDS_HITS // 2 if volume <= OC.HALF_VOXELS else OC.LDS_HITS
            if site == "maxchunk":
                # first under kRfExcludeSample: counts alone, the walk's own apply at a full chunk; then with samples,
                # more than the walk stages -- the deferred route at the largest counts
                assert not samples[0] and most_samples > lds_hits, sheet.name
            elif site != "dense":
                assert most_samples <= lds_hits, sheet.name       # no deferred events beside the dense site
            counts = [n for s in segments for n in s.values()]
            one_chunk, several = all(n <= sheet.chunk for n in counts), all(n > sheet.chunk for n in counts)
            if site in ("walk", "lists", "dense", "half", "tiled", "spill", "maxchunk"):
                assert sheet.layers == ("occupancy",), sheet.name  # inline sample replay: no other layer
            if site == "walk":
                assert one_chunk and volume % 4 == 0 and OC.HALF_VOXELS < volume <= OC.TILE_VOXELS, sheet.name
            if site == "lists":
                assert several and volume % 4 == 0 and OC.HALF_VOXELS < volume <= OC.TILE_VOXELS, sheet.name
            if site == "dense":
                assert most_samples > lds_hits and volume > OC.HALF_VOXELS, sheet.name
            if site == "half":
                assert volume <= OC.HALF_VOXELS and volume % 4 == 0 and (one_chunk or several or "count" in sheet.name)
            if site == "tiled":
                assert volume > OC.TILE_VOXELS and (one_chunk or several), sheet.name
                slabs = {sheet.mp.local(c.target[1])[2] // 12 for c in sheet.cells}
                assert slabs == {0, 1, 2, 3}, sheet.name          # every z slab of the 48^3 region holds targets
            if site == "spill":
                assert len(sheet.regions()) + 4 > 4 >= len(sheet.regions()), sheet.name
            if site == "maxchunk":
                assert sheet.chunk == OC.MAX_CHUNK and {OC.MAX_CHUNK, OC.MAX_CHUNK + 1} <= set(counts), sheet.name
        names = [s.name for s in sheets[site]]
        if site == "mean":
            assert all(s.layers == OC.MEAN for s in sheets[site])
            assert any("/walk" in n for n in names) and any("/lists" in n for n in names)
            count = [s for s in sheets[site] if s.name.startswith("count/")][0]
            assert sorted(count.segments(0).values()) == [OC.N, OC.N, OC.N + 1, OC.N + 1]
        if site == "odd":
            volumes = {s.mp.volume for s in sheets[site]}
            assert any(v % 2 == 1 and v > OC.HALF_VOXELS for v in volumes)          # scalar branches, full shape
            assert any(v % 4 == 2 and v > OC.HALF_VOXELS for v in volumes)
            assert any(v % 2 == 1 and v <= OC.HALF_VOXELS for v in volumes)         # and the half shape
            for dim in OC.ODD_DIMS:
                mine = [s for s in sheets[site] if s.mp.dim == dim]
                assert {s.layers for s in mine} == {("occupancy",), OC.MEAN}
                assert any("/walk" in s.name for s in mine) and any("/lists" in s.name for s in mine)
        if site == "stop":
            assert {s.layers for s in sheets[site]} == {("occupancy",), OC.MEAN}
        if site in ("walk", "lists"):
            count = [s for s in sheets[site] if s.name.startswith("count/")][0]
            assert set(count.segments(0).values()) == {OC.N if site == "walk" else OC.N + 1}
    # samples and plain counts share a 4-voxel group and a mask word (the lists site's two parts meet there)
    sheet = [s for s in sheets["lists"] if s.name.startswith("states/default")][0]
    kinds = {}
    for e in sheet.events[0]:
        kinds.setdefault(e.key, set()).add(e.kind)
    groups = {}
    for (region, vi), k in kinds.items():
        groups.setdefault((region, vi // 4), []).append(k)
    assert any({"h"} in g and {"m"} in g and {"m", "h"} in g for g in groups.values())


def changed(a, b):
    return any(set(x) != set(y) or any((x[r].view(np.uint32) != y[r].view(np.uint32)).any() for r in x)
               for x, y in zip(a, b))


def test_every_mutant_is_killed_on_every_site_it_applies_to(sheets, capsys):
    assert set(APPLIES) == set(OC.SITES)
    assert {m for site in APPLIES.values() for m in site} == set(O.MUTANTS)          # every mutant applies somewhere
    table = []
    for site in OC.SITES:
        for mutant in APPLIES[site]:
            killer = next((s.name for s in sheets[site] if changed(s.mutant_states(mutant), s.states)), None)
            assert killer is not None, (site, mutant)
            table.append("%-9s %-28s %s" % (site, mutant, killer))
    with capsys.disabled():
        print("\n" + "\n".join(table))
