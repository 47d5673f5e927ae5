"""CPU: the exact model of the TSDF voxel update (tests/tsdf_ref.py) against its own rational evaluation, the oracle and
the reference header compiled in place, on the constructed sheets of tests/tsdf_cases.py -- and the conditions those
sheets have to meet for the GPU test (tests/test_gpu_tsdf_states.py) to mean anything: every edge is reached (counts
printed by test_conditions_on_the_sheets), no sheet discards more than a tenth of what it drew, every option-change
script leaves the oracle off the counting shortcut's answer in a voxel that saw free-space visits only, and every
mutant of the model is killed on every site."""
import ctypes as C
import os

import numpy as np
import pytest

import tsdf_cases
import tsdf_ref
from oracle import oracle as O
from tsdf_cases import CHANGES, COUNTS, FREE_MARGIN, HOLES, REGION, SITES, VARIANTS, differing, ordinal, replay, shortcut
from tsdf_ref import F, bits, same, update_exact, update_ref

_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
ref = None
if os.path.exists(O.REF_LIB_PATH):
    ref = C.CDLL(O.REF_LIB_PATH)
    ref.ref_calculate_tsdf.restype = C.c_int
    ref.ref_calculate_tsdf.argtypes = [_dp, _dp, _dp, C.c_float, C.c_float, C.c_float, C.c_float, _fp, _fp]


@pytest.fixture(scope="module")
def sheets():
    return tsdf_cases.build()


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def _through(fn, o, sensor, sample, centre, w, d):
    cw, cd = C.c_float(float(w)), C.c_float(float(d))
    fn(_d3(sensor), _d3(sample), _d3(centre), o.trunc, o.max_weight, o.dropoff, o.sparsity, C.byref(cw), C.byref(cd))
    return F(cw.value), F(cd.value)


def check_one(o, sensor, sample, centre, w, d, with_ref=True):
    sdf = tsdf_ref.sdf_ref(sensor, sample, centre)
    got = update_ref(o, sdf, w, d)
    exact = update_exact(o, sdf, w, d)
    assert same(got[0], exact[0]) and same(got[1], exact[1]), ("update_ref != update_exact", o, sdf, w, d, got, exact)
    theirs = _through(O.lib.oracle_calculate_tsdf, o, sensor, sample, centre, w, d)
    assert same(got[0], theirs[0]) and same(got[1], theirs[1]), ("update_ref != oracle", o, sdf, w, d, got, theirs)
    if ref is not None and with_ref:
        theirs = _through(ref.ref_calculate_tsdf, o, sensor, sample, centre, w, d)
        assert same(got[0], theirs[0]) and same(got[1], theirs[1]), ("update_ref != reference", o, sdf, w, d, got, theirs)


def test_round_f32_is_the_ieee_rounding():
    """round_f32 against the C library's double -> float conversion on doubles (exact rationals) around every kind of
    boundary: ties, subnormals, the overflow threshold."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    xs = list(rng.standard_normal(2000) * 10.0 ** rng.integers(-50, 39, 2000))
    for base in (1.0, 0.3, 2.0 ** -126, 2.0 ** -149, 2.0 ** -140, 3.4028234e38, 2.0 ** 24):
        b = float(F(base))
        for k in range(1, 8):
            ulp = b - float(np.nextafter(F(b), F(0)))
            xs += [b + ulp * k / 8.0, b - ulp * k / 16.0, -(b + ulp * k / 8.0)]
    xs += [3.4028235677973366e38, 3.4028235677973362e38, 2.0 ** -150, 2.0 ** -150 * 1.0000001, 2.0 ** -151]
    for x in xs:
        with np.errstate(all="ignore"):
            want = F(x)
        assert bits(F(tsdf_ref.round_f32(Fraction(x)))) == bits(want), x


def test_model_on_every_aimed_visit_and_a_random_sweep(sheets):
    """update_ref == update_exact == oracle_calculate_tsdf (== the reference header where it is built), bit for bit (any
    NaN for any NaN): on the state every aimed ray meets in its voxel, on a sample of all other visits, and on a seeded
    sweep of planted weights x planted distances x sdf x every option set."""
    checked = 0
    rng = np.random.default_rng(11)
    for sheet in sheets:
        if sheet.site not in ("direct", "replay"):
            continue                                   # the other sites repeat these scripts in other geometry
        geo = sheet.geo
        before = (sheet.w0, sheet.d0)
        aimed = {}
        for ci, vi, _ in sheet.aimed:
            aimed.setdefault(ci, set()).add(vi)
        for ci, call in enumerate(sheet.calls):
            seen = set()
            extra = set(rng.choice(len(call.vi), 60, replace=False).tolist())
            for i in range(len(call.vi)):
                vi = int(call.vi[i])
                if vi in seen:
                    continue                            # the voxel's first visit of the call: its state is `before`
                seen.add(vi)
                if vi in aimed.get(ci, ()) or i in extra:
                    r = int(call.ray[i])
                    check_one(call.opts, call.rays[2 * r], call.rays[2 * r + 1], geo.centre(vi), before[0][vi],
                              before[1][vi], with_ref=checked % 4 == 0)
                    checked += 1
            before = sheet.states[ci]
    all_opts = sorted({o for script in VARIANTS.values() for o in script if isinstance(o, tsdf_ref.Opts)})
    swept = 0
    for o in all_opts:
        weights, distances = tsdf_cases.planted_weights(o.max_weight), tsdf_cases.planted_distances(o.trunc)
        t = float(o.trunc)
        for cut in (3.0 * t, 1.0101 * t, 1.0000001 * t, 0.5 * t, 1e-9, 0.0, -1e-9, -0.5 * t, -1.0000001 * t, -1.5 * t):
            g = float(rng.uniform(0.5, 3.0))
            sensor, sample, centre = (0.0, 0.0, 0.0), (g, 0.0, 0.0), (g - cut, float(rng.uniform(-0.01, 0.01)), 0.0)
            for w in weights:
                for d in distances:
                    check_one(o, sensor, sample, centre, F(w), d, with_ref=swept % 8 == 0)
                    swept += 1
    print("\nmodel == exact == oracle%s: %d aimed and sampled visits, %d swept" % (
        " == reference" if ref is not None else "", checked, swept))
    assert checked > 3000 and swept > 10000 and len(all_opts) >= 12


def test_scripts_through_the_oracle_mapper(sheets):
    """Every sheet through OracleMap.integrate_tsdf, call by call with the option changes in between: the whole region
    equals the model's replay over the oracle's own walk order after every call, and one call per segment gives the
    same."""
    for sheet in sheets:
        om = tsdf_cases.make_oracle(sheet)
        for call, state in zip(sheet.calls, sheet.states):
            tsdf_cases.set_options(om, call.opts)
            om.integrate_tsdf(call.rays)
            got = tsdf_cases.state_of(om.region_layer(REGION, "tsdf"))
            assert len(differing(state, got)) == 0, (sheet.name, differing(state, got)[:8])
        assert [tuple(k) for k in om.region_keys()] == [REGION], sheet.name
        merged = tsdf_cases.make_oracle(sheet)
        for o, _, rays in tsdf_cases.batches(sheet, merged=True):
            tsdf_cases.set_options(merged, o)
            merged.integrate_tsdf(rays)
        assert len(differing(sheet.states[-1], tsdf_cases.state_of(merged.region_layer(REGION, "tsdf")))) == 0


def reach(sheet):
    """Edge name -> how often the sheet lands on it; the free-space-only runs of the last segment that the oracle does not
    leave at the counting shortcut's answer; and those of them in voxels that were planted countable and never saw a
    visit near the surface -- what they hold, the script itself made."""
    record, trace = [], {}
    replay(sheet, record=record, trace=trace)
    out = dict(("path " + k, v) for k, v in trace.items())
    first = record[0]
    for w in tsdf_cases.planted_weights(sheet.calls[0].opts.max_weight):
        key = "weight %r" % float(F(w))
        out[key] = int(np.count_nonzero(bits(first["w0"]) == bits(F(w))))
    for d in tsdf_cases.planted_distances(sheet.calls[0].opts.trunc):
        name = "distance %s" % ("nan" if d != d else repr(float(d) / float(sheet.calls[0].opts.trunc)) + " trunc")
        out[name] = int(np.count_nonzero(bits(first["d0"]) == bits(d)))
    out["state unobserved (0, 0)"] = int(np.count_nonzero((bits(first["w0"]) == 0) & (bits(first["d0"]) == 0)))
    out["state (0, -0.0)"] = int(np.count_nonzero((bits(first["w0"]) == 0) & (bits(first["d0"]) == 0x80000000)))
    off = off_script = free_groups = 0
    ordinary = ((sheet.w0 == np.trunc(sheet.w0)) & (sheet.w0 >= 0) & (sheet.w0 <= 1e4)
                & ((sheet.d0 == sheet.calls[0].opts.trunc) | ((sheet.w0 == 0) & (sheet.d0 == 0))))
    last_segment = sheet.calls[-1].segment
    met_surface = np.zeros(sheet.volume, dtype=bool)      # voxels some earlier visit came near the surface in
    for call, entry in zip(sheet.calls, record):
        o = entry["opts"]
        s = entry["sdf"]
        with np.errstate(all="ignore"):
            for name, target in (("margin", FREE_MARGIN * o.trunc), ("trunc", o.trunc), ("-trunc", -o.trunc)):
                k = ordinal(s) - int(ordinal(target))
                k = np.where(np.isnan(s), 99, k)
                for label, hit in (("-", (k < 0) & (k >= -4)), ("=", k == 0), ("+", (k > 0) & (k <= 4))):
                    key = "sdf %s %s" % (name, label)
                    out[key] = out.get(key, 0) + int(np.count_nonzero(hit))
            for key, hit in (("sdf 0 -", (s < 0) & (s > F(-1e-6))), ("sdf 0 =", s == 0), ("sdf 0 +", (s > 0) & (s < F(1e-6))),
                             ("sdf free (>= 2 trunc)", s >= F(2) * o.trunc), ("sdf behind (< 0)", s < 0),
                             ("sdf below -trunc", s < -o.trunc), ("sdf inside (0.2 .. 0.8 trunc)",
                                                                   (s > F(0.2) * o.trunc) & (s < F(0.8) * o.trunc))):
                out[key] = out.get(key, 0) + int(np.count_nonzero(hit))
        free = entry["free"]
        cw, cd = shortcut(entry)
        not_counted = free & ~(same(entry["w1"], cw) & same(entry["d1"], cd) & ~np.isnan(entry["w1"]))
        free_groups += int(np.count_nonzero(free))
        for n in COUNTS:
            key = "free-space only, n = %d" % n
            out[key] = out.get(key, 0) + int(np.count_nonzero(free & (entry["n"] == n)))
        out["free-space only, countable"] = out.get("free-space only, countable", 0) + int(
            np.count_nonzero(free & ~not_counted))
        if call.segment == last_segment:
            off += int(np.count_nonzero(not_counted))
            off_script += int(np.count_nonzero(not_counted & ordinary[entry["vi"]] & ~met_surface[entry["vi"]]))
        met_surface[entry["vi"][~free]] = True
    out["free-space only"] = free_groups
    return out, off, off_script, record


def test_counted_is_the_shortcut_predicate(sheets):
    """tsdf_ref.counted (a scalar replay) says what the sheets' bulk comparison says, on a sample of free-space runs."""
    sheet = next(s for s in sheets if s.name == "direct/drop_on_off")
    record = []
    replay(sheet, record=record)
    rng = np.random.default_rng(2)
    yes = no = 0
    for entry in record:
        cw, cd = shortcut(entry)
        bulk = same(entry["w1"], cw) & same(entry["d1"], cd) & ~np.isnan(entry["w1"])
        groups = np.flatnonzero(entry["free"])
        for g in rng.choice(groups, min(60, len(groups)), replace=False):
            a = entry["starts"][g]
            sdfs = entry["sdf"][a:a + entry["n"][g]]
            said = tsdf_ref.counted(entry["opts"], entry["w0"][g], entry["d0"][g], sdfs)
            assert said == bool(bulk[g]), (entry["w0"][g], entry["d0"][g], len(sdfs))
            yes, no = yes + said, no + (not said)
    assert yes >= 20 and no >= 20, (yes, no)


def test_conditions_on_the_sheets(sheets, capsys):
    total, lines = {}, []
    for sheet in sheets:
        out, off, off_script, _ = reach(sheet)
        assert 10 * sheet.discarded <= sheet.drawn, (sheet.name, sheet.discarded, sheet.drawn)
        rays = [len(c.rays) // 2 for c in sheet.calls]
        if sheet.site == "direct":
            assert max(rays) <= tsdf_cases.CHUNK_RAYS, (sheet.name, rays)
        else:
            # (the calls after the last option change: the ones that apply counts to what the earlier options left)
            late = [n for n, c in zip(rays, sheet.calls) if c.segment == sheet.calls[-1].segment]
            assert min(late) > tsdf_cases.CHUNK_RAYS, (sheet.name, rays)
        # a voxel that saw free-space visits only and that the oracle does NOT leave at (min(w + n, max), trunc)
        assert off >= 1, sheet.name
        if sheet.variant in HOLES:
            assert off_script >= 1, (sheet.name, "no voxel the script itself made uncountable")
        for n in COUNTS:
            assert out["free-space only, n = %d" % n] >= 1, (sheet.name, n)
        assert out["free-space only, countable"] >= 1, sheet.name
        lines.append("%-34s rays/call %-22s discarded %d of %d; free-space-only runs %d, off the shortcut in the last "
                     "segment %d (%d from the script's own states)" % (
                         sheet.name, rays, sheet.discarded, sheet.drawn, out["free-space only"], off, off_script))
        for key, n in out.items():
            total[(sheet.site, key)] = total.get((sheet.site, key), 0) + n
        if sheet.site == "tiled":
            slab = tsdf_cases.slab_layers(sheet.dim)
            assert len({z // slab for _, z in sheet.free_rows}) >= 2 and len({z // slab for _, z in sheet.edge_rows}) >= 2
    assert {s.variant for s in sheets if s.site == "direct"} >= set(CHANGES) | set(HOLES)
    default, reverse = (next(s for s in sheets if s.name == "direct/" + v) for v in ("default", "reversed"))
    # the reversed copy: same planted region, every call's rays in the opposite order -- the model tells them apart
    back = tsdf_cases.Sheet("direct", "reversed")
    back.w0, back.d0 = reverse.w0, reverse.d0
    back.calls = [c._replace(vi=c.vi[::-1], sdf=c.sdf[::-1], sdf_late=c.sdf_late[::-1], ray=c.ray[::-1])
                  for c in reverse.calls]
    told_apart = len(differing(replay(back)[-1], reverse.states[-1]))
    assert told_apart >= 16, told_apart
    assert default.variant == "default"
    keys = sorted({k for _, k in total})
    with capsys.disabled():
        print("\n" + "\n".join(lines))
        print("order: %d voxels of direct/reversed end elsewhere when its rays are replayed in the opposite order" %
              told_apart)
        print("\nvisits (or planted voxels met) per edge and site")
        print("%-34s %s" % ("edge", " ".join("%8s" % s for s in SITES)))
        for k in keys:
            print("%-34s %s" % (k, " ".join("%8d" % total.get((s, k), 0) for s in SITES)))
    for k in keys:
        for s in SITES:
            if s == "replay" and k == "distance 1.0 trunc":
                continue                           # the replay site plants no voxel at the truncation distance
            if s != "direct" and (s, k) not in total:
                continue                           # a planted max_weight of a variant only `direct` runs
            assert total.get((s, k), 0) >= 1, (s, k)


def test_every_mutant_is_killed_on_every_site(sheets, capsys):
    """Voxels whose final state a mutant changes, per site.  Every mutant runs on every site (the ordered replay runs
    wherever a voxel is flagged; count_once is what the sites other than `replay` do where the mask lets them) and has
    to be killed there."""
    table = {}
    for sheet in sheets:
        for m in tsdf_ref.MUTANTS:
            kills = len(differing(replay(sheet, mutant=m)[-1], sheet.states[-1]))
            table[(m, sheet.site)] = table.get((m, sheet.site), 0) + kills
    with capsys.disabled():
        print("\nvoxels killed per (mutant, site)")
        print("%-18s %s" % ("mutant", " ".join("%8s" % s for s in SITES)))
        for m in tsdf_ref.MUTANTS:
            print("%-18s %s" % (m, " ".join("%8d" % table[(m, s)] for s in SITES)))
    for (m, site), kills in table.items():
        assert kills >= 1, (m, site)
