"""CPU: the traversal model (tests/traversal_ref.py) and its sheets (tests/traversal_cases.py).

  * visits / cpu_adds against the oracle: every distinct sheet ray alone in a fresh oracle map holds, voxel by voxel,
    exactly the float32 the model says (uint32 views), and the oracle's own walk reports the model's voxels, enter and
    exit ranges (float64, exact);
  * visits against the independent exact walker (tests/exact_walk.py) on every lattice ray of the 2^-4 m sheets;
  * the oracle, fed each sheet call by call, equals the running float32 sum of cpu_adds bit for bit and therefore stays
    within (n + s) * ulp(max |partial sum|) / 2 of the exact sum;
  * the model stays within n * 2^-(unit_bits + 1) + (b + s) * ulp / 2 of it (both bounds derived in traversal_ref);
  * the edges the sheets were built for are reached;
  * every mutant is caught on every site it applies to, and stays within the old rtol = 1e-5, atol = 1e-6 on a sheet
    on which it is caught.

Where a mutant cannot apply (INAPPLICABLE): a site none of whose sheets can tell it from the model, by construction."""
from fractions import Fraction

import numpy as np
import pytest

import exact_walk
import traversal_cases as TC
import traversal_ref as T
from oracle.oracle import OracleMap
from traversal_ref import F

# mutant -> {site: why no sheet of the site can show it}
_FLAGS0 = "the site's mapper is fed default ray flags only"
_ONE_CHUNK = "every region's segments fit one walk chunk, so per chunk is per batch"
_NO_REWALK = "the walk is never repeated"
_NO_WRAP = "no sheet of the site brings a tile word to exactly 2^32"
INAPPLICABLE = {
    "truncate": {},
    "unit_27_always": {},
    "carry_lost_on_exact_wrap": {"stop": _NO_WRAP, "rewalk": _NO_WRAP,
                                 "chunks": "which visits share a word is the device's cut of the region's segments"},
    "fold_per_chunk": {s: _ONE_CHUNK for s in TC.SITES if s != "chunks"},
    "fold_before_samples": {},
    "end_exits_at_step_time": {s: _FLAGS0 for s in ("chunks", "stop", "ndt", "rewalk", "tiled", "spill")},
    "origin_range_not_passed": {s: _FLAGS0 for s in ("chunks", "stop", "ndt", "rewalk", "tiled", "spill")},
    "entry_time_min_axis": {"stop": "its one sheet stays inside region (0, 0, 0)"},
    "last_exit_across_calls": {"stop": "every call's first ray reports a voxel",
                               "chunks": "every call's first ray reports a voxel"},
    "pass_twice_on_rewalk": {s: _NO_REWALK for s in TC.SITES if s != "rewalk"},
}


@pytest.fixture(scope="module")
def sheets():
    return TC.all_sheets()                           # [(sheet, [sites])]


def bits(a):
    return np.asarray(a, dtype=F).view(np.uint32)


def make_oracle(sheet):
    return TC.make_oracle(sheet, ("occupancy", "traversal"))


def distinct_rays(sheets):
    seen, out = set(), []
    for sheet, _ in sheets:
        for call in sheet.calls:
            if call.flags & T.RF_STOP_ON_FIRST_OCCUPIED:
                continue                             # (alone in a fresh map nothing is occupied: the flag does nothing)
            for r in range(call.rays.shape[0] // 2):
                ray = call.rays[2 * r:2 * r + 2]
                key = (sheet.mp.res, sheet.mp.dim, call.flags, ray.tobytes())
                if key not in seen:
                    seen.add(key)
                    out.append((sheet.mp, call.flags, ray))
    return out


def test_every_ray_alone_matches_the_oracle(sheets):
    rays = distinct_rays(sheets)
    assert len(rays) > 3000
    walkers = {}
    for mp, flags, ray in rays:
        adds, _ = T.cpu_adds(T.Call(ray, flags), mp)
        want = {}
        for a in adds:
            tile = want.setdefault(a.region, np.zeros(mp.volume, dtype=F))
            tile[a.vi] = F(tile[a.vi] + a.value)
        om = OracleMap(mp.res, mp.dim, ("occupancy", "traversal"))
        om.integrate_occupancy(ray, flags=flags)
        got = om.chunks(["traversal"])
        for region, tile in want.items():
            assert region in got, (ray, flags, region)
            assert np.array_equal(bits(got[region]["traversal"]), bits(tile)), (ray.tolist(), flags, region)
        for region, layers in got.items():
            if region not in want:
                assert not layers["traversal"].any(), (ray.tolist(), flags, region)
        # the oracle's own walk: the same voxels, the same float64 ranges
        if not flags & T.RF_EXCLUDE_RAY:
            walker = walkers.setdefault((mp.res, mp.dim), OracleMap(mp.res, mp.dim, ("occupancy",)))
            walk_flags = (0 if flags & T.RF_END_POINT_AS_FREE else 2) | (1 if flags & T.RF_EXCLUDE_ORIGIN else 0)
            keys, enter, exit_ = walker.walk(ray[0], ray[1], walk_flags)
            v = T.visits(ray[0], ray[1], flags, mp)
            assert [(k[0], mp.index(k[1])) for k in keys] == v.keys, (ray.tolist(), flags)
            assert np.array_equal(np.array(enter).view(np.uint64), np.array(v.enter, dtype=np.float64).view(np.uint64))
            assert np.array_equal(np.array(exit_).view(np.uint64), np.array(v.exit, dtype=np.float64).view(np.uint64))


def test_visits_against_the_exact_walker(sheets):
    """Every ray of the 2^-4 m sheets whose coordinates lie on the 2^-33 m lattice: the voxel sequence of the exact
    rational walker (start and end voxel included, as under kRfEndPointAsFree)."""
    sub = 1 << 29                                    # lattice units per 2^-4 m voxel
    walked = undecidable = 0
    for mp, flags, ray in distinct_rays(sheets):
        if mp.res != TC.FINE or mp.dim[0] % 2 or flags & (T.RF_EXCLUDE_RAY | T.RF_EXCLUDE_ORIGIN):
            continue
        units = ray * 2.0 ** 33
        if not np.array_equal(units, np.floor(units)) or np.array_equal(ray[0], ray[1]):
            continue
        s, e = [int(v) for v in units[0]], [int(v) for v in units[1]]
        try:
            # (exact_walk counts voxels from the origin; region (0, 0, 0) is centred on it)
            want = exact_walk.walk(s, e, sub=sub, region=mp.dim)
        except exact_walk.Undecidable:
            undecidable += 1
            continue
        got = T.visits(ray[0], ray[1], T.RF_END_POINT_AS_FREE, mp).keys
        assert [(r, mp.index(l)) for r, l in want] == got, ray.tolist()
        walked += 1
    assert walked > 100 and undecidable == 0, (walked, undecidable)


def voxel_adds(sheet):
    """(region, vi) -> [[adds of call 0], [adds of call 1], ...] in the CPU's order."""
    out, occupancy = {}, sheet.occupancy()
    for k, call in enumerate(sheet.calls):
        adds, _ = T.cpu_adds(call, sheet.mp, occupancy)
        for a in adds:
            out.setdefault((a.region, a.vi), [[] for _ in sheet.calls])[k].append(a)
    return out


def planted_value(sheet, key):
    tile = sheet.planted.get(key[0])
    return F(0.0) if tile is None else tile[key[1]]


def test_oracle_and_model_stay_within_their_bounds(sheets):
    worst_oracle = worst_model = 0.0
    for sheet, _ in sheets:
        mp = sheet.mp
        unit_bits = T.traversal_unit_bits(mp.res)
        per_voxel = voxel_adds(sheet)
        om = make_oracle(sheet)
        running = {r: t.copy() for r, t in sheet.planted.items()}
        peak_cpu = {}
        for k, call in enumerate(sheet.calls):
            om.integrate_occupancy(call.rays, flags=call.flags)
            for key, calls in per_voxel.items():
                tile = running.setdefault(key[0], np.zeros(mp.volume, dtype=F))
                peak = max(peak_cpu.get(key, 0.0), abs(float(tile[key[1]])))
                for a in calls[k]:
                    tile[key[1]] = F(tile[key[1]] + a.value)
                    peak = max(peak, abs(float(tile[key[1]])))
                peak_cpu[key] = peak
            got = om.chunks(["traversal"])
            for region, tile in running.items():
                have = got[region]["traversal"] if region in got else np.zeros(mp.volume, dtype=F)
                assert np.array_equal(bits(have), bits(tile)), (sheet.name, k, region)
        for key, calls in per_voxel.items():
            flat = [a for c in calls for a in c]
            n = sum(1 for a in flat if not a.share)
            s = len(flat) - n
            exact = T.exact_sum([planted_value(sheet, key)] + [a.value for a in flat])
            # the oracle
            err = abs(Fraction(float(running[key[0]][key[1]])) - exact)
            bound = Fraction(n + s) * Fraction(T.ulp32(peak_cpu[key])) / 2
            assert err <= bound, (sheet.name, key, float(err), float(bound))
            worst_oracle = max(worst_oracle, float(err / bound) if bound else 0.0)
            # the model
            details = [d.get(key, {}) for d in sheet.details]
            assert all(d.get("fold_exact", True) for d in details), (sheet.name, key)
            for a in flat:
                # (a visit add that the conversion clamps to 0 units is within half a unit of 0 anyway)
                assert a.share or (a.value == a.value and float(a.value) > -2.0 ** -(unit_bits + 1)), (sheet.name, a)
                assert a.share or float(a.value) * 2.0 ** unit_bits < 2.0 ** 31, (sheet.name, a)
            b = sum(1 for d in details if sum(d.get("units", ())) > 0)
            peak = max([d.get("peak", 0.0) for d in details])
            err = abs(Fraction(float(sheet.states[-1][key[0]][key[1]])) - exact)
            bound = Fraction(n, 1 << (unit_bits + 1)) + Fraction(b + s) * Fraction(T.ulp32(peak)) / 2
            assert err <= bound, (sheet.name, key, float(err), float(bound), n, s, b)
            worst_model = max(worst_model, float(err / bound) if bound else 0.0)
    assert 0 < worst_oracle <= 1 and 0 < worst_model <= 1


def site_details(sheets, site):
    for sheet, sites in sheets:
        if site in sites:
            for k, detail in enumerate(sheet.details):
                for key, d in detail.items():
                    yield sheet, k, key, d


def test_every_edge_is_reached(sheets):
    by_name = {sheet.name: sheet for sheet, _ in sheets}
    # unit_bits and the threshold 8 / sqrt(3) m
    assert [T.traversal_unit_bits(r) for r in (2.0 ** -4, 0.1, 0.37, 4.5, 4.6188, 4.6189, 4.75, 10.0)] == [
        28, 28, 28, 28, 28, 27, 27, 26]
    assert {T.traversal_unit_bits(s.mp.res) for s, sites in sheets if "direct" in sites} == {28, 27, 26}
    # ties and near ties of the conversion
    assert [T.units_of(F(k * 2.0 ** -29), 28) for k in (1, 3, 5)] == [0, 2, 2]
    assert T.units_of(F(-1.0), 28) == 0 and T.units_of(F(np.nan), 28) == 0 and T.units_of(F(1e-16), 28) == 0
    tiny = by_name["tiny_start/0.0625/32x32x32"]
    adds = [a.value for call in tiny.calls for a in T.cpu_adds(call, tiny.mp)[0] if not a.share]
    for k in (1, 3, 5):
        assert F(k * 2.0 ** -29) in adds
    assert any(0.9 < float(a) * 2.0 ** 28 < 1.0 for a in adds)
    assert max(adds) < 2e-7                                           # every visit of the sheet is tiny
    fine = [a for s in (tiny, by_name["tiny_start/0.1/32x32x32"]) for call in s.calls
            for a in T.cpu_adds(call, s.mp)[0] if not a.share]
    assert any(0 < float(a.value) < 1e-15 for a in fine)               # the start-on-a-wall visit
    ends = by_name["tiny_end/0.0625/32x32x32"]
    end_adds = [a for call in ends.calls for a in T.cpu_adds(call, ends.mp)[0]]
    assert all(not a.share for a in end_adds)
    flagged = [a for n in TC.FLAG_SETS if "end_as_free" in n for call in by_name["flags/" + n].calls
               for a in T.cpu_adds(call, by_name["flags/" + n].mp)[0]]
    assert any(not a.share and abs(float(a.value)) < 1e-15 for a in flagged + end_adds)    # an end point on a wall
    # near-diagonal visits at 4.5 m: just under 2^31 units
    top = max(n for _, _, _, d in site_details(sheets, "direct") for n in d.get("units", ()))
    assert 0.97 * 2 ** 31 < top < 2 ** 31
    # words that end at exactly 0 after one and after two carries; words that wrap without landing on 0
    for site in ("direct", "mean", "ndt", "tiled", "spill"):
        words = [w for _, _, _, d in site_details(sheets, site) for w in d.get("words", {}).values()]
        assert any(w.word == 0 and w.carries == 1 for w in words), site
        assert any(w.word == 0 and w.carries == 2 for w in words), site
        assert any(w.word != 0 and w.carries >= 1 for w in words), site
        assert any(w.word == 0xff000000 and w.carries == 0 for w in words), site      # 255 visits: one short of it
    # ... and the same sums spread over several chunks
    multi = [d for _, _, _, d in site_details(sheets, "chunks") if len(d.get("words", {})) > 1]
    assert any(sum(d["units"]) == 1 << 32 for d in multi) and any(sum(d["units"]) == 1 << 33 for d in multi)
    for sheet, sites in sheets:
        through = max(len({a.ray for a in T.cpu_adds(c, sheet.mp)[0] if a.region == (0, 0, 0) and not a.share})
                      for c in sheet.calls)
        assert (through > T.CHUNK_RAYS) == (sites == ["chunks"]), (sheet.name, through)
        assert all(c.rays.shape[0] // 2 <= 16384 for c in sheet.calls)
    # more than 16 m into one voxel in one call, from unequal lengths
    assert any(sum(d["units"]) > 16 << 28 and len(set(d["units"])) > 100
               for _, _, _, d in site_details(sheets, "direct") if "units" in d)
    # a voxel holding >= 2^10 m that receives a batch below half its ulp, and keeps it or loses it
    small = [(s, k, key, d) for s, k, key, d in site_details(sheets, "direct")
             if 0 < sum(d.get("units", ())) * 2.0 ** -28 < T.ulp32(d["peak"]) / 2 and d["peak"] >= 2.0 ** 10]
    assert len(small) > 100
    # samples and visits in the same voxel in the same call
    assert sum(1 for _, _, _, d in site_details(sheets, "direct") if d.get("n", 0) and d.get("s", 0)) > 100
    # the same rays as 1, 2, 3 and 6 calls: the model's answers differ from one another
    folds = [by_name["fold/0.1/32x32x32/%dcalls" % k] for k in (1, 2, 3, 6)]
    finals = [np.concatenate([bits(s.states[-1][r]) for r in sorted(s.states[-1])]) for s in folds]
    assert all(not np.array_equal(finals[i], finals[j]) for i in range(4) for j in range(i))
    # negative shares, inherited exit ranges, a first ray that reports nothing
    for name in ("flags/none", "flags/end_as_free", "flags/exclude_sample"):
        sheet = by_name[name]
        for call in sheet.calls:
            first = T.visits(call.rays[0], call.rays[1], call.flags, sheet.mp)
            assert not first.reported or call.flags & T.RF_END_POINT_AS_FREE
    none = by_name["flags/none"]
    shares = [a for call in none.calls for a in T.cpu_adds(call, none.mp)[0] if a.share]
    assert sum(1 for a in shares if a.value < 0) >= 20
    # a stopped ray: fewer shares than rays
    stop = by_name["stop/wall"]
    n_rays = sum(c.rays.shape[0] // 2 for c in stop.calls)
    occupancy = stop.occupancy()
    n_shares = sum(1 for c in stop.calls for a in T.cpu_adds(c, stop.mp, occupancy)[0] if a.share)
    assert n_rays // 4 < n_shares < 3 * n_rays // 4
    # region entry by an x, a y and a z step, through an edge and a corner
    entry = by_name["entry/0.0625/32x32x32"]
    assert len(entry.regions()) == 8


def old_bar(a, b):
    regions = set(a) | set(b)
    zero = None
    for r in regions:
        x, y = a.get(r, zero), b.get(r, zero)
        if x is None or y is None:
            other = x if y is None else y
            if not np.allclose(other, 0, rtol=1e-5, atol=1e-6):
                return False
            continue
        if not np.allclose(x, y, rtol=1e-5, atol=1e-6):
            return False
    return True


def same_bits(a, b):
    for r in set(a) | set(b):
        x, y = a.get(r), b.get(r)
        if x is None or y is None:
            if (x if y is None else y).any():
                return False
        elif not np.array_equal(bits(x), bits(y)):
            return False
    return True


def test_every_mutant_is_caught_and_was_invisible(sheets, capsys):
    table = {}
    for mutant in T.MUTANTS:
        caught, hidden = {}, []
        for sheet, sites in sheets:
            states = sheet.mutant_states(mutant)
            differs = any(not same_bits(m, s) for m, s in zip(states, sheet.states))
            if differs:
                for site in sites:
                    caught.setdefault(site, []).append(sheet.name)
                if all(old_bar(m, s) for m, s in zip(states, sheet.states)):
                    hidden.append(sheet.name)
        for site in TC.SITES:
            if site in INAPPLICABLE[mutant]:
                assert site not in caught, (mutant, site, "listed as inapplicable but caught", caught[site])
            else:
                assert site in caught, (mutant, site)
        assert hidden, (mutant, "no sheet on which the old tolerance passes it")
        table[mutant] = (caught, hidden)
    with capsys.disabled():
        print()
        for mutant, (caught, hidden) in table.items():
            print("%-26s caught on %-60s within 1e-5 on %d sheets" % (mutant, ",".join(sorted(caught)), len(hidden)))
