"""CPU restatement of the layered heightmaps, ohm::Heightmap::buildHeightmap in HeightmapMode::kLayeredFill and
kLayeredFillUnordered -- TEST INFRASTRUCTURE.  The device build (ohmhip_map_heightmap_layered) is held to it at exact
equality: every slot, every field, the visit log and the stats.

Written from the reference line by line (ohmheightmap/Heightmap.cpp:391-402, 522-835; PlaneFillLayeredWalker.cpp;
private/HeightmapOperations.cpp:32-62, 135-165, 515-773); the rule numbers L1-L7 are those of the layered block of
include/ohmhip.h, rules 1, 3, 4 and 5 those of the heightmap block, taken from tests/heightmap_ref.py, the extents and
the seed (F1, F2) from tests/heightmap_fill_ref.py.

build_layered()              the reference as written: one std::deque, one visit at a time
build_layered_generations()  the same walk one generation of the queue at a time: the offers of a generation replayed
                             per grid cell, its adds per heightmap cell, both in key order -- the device formulation"""
from collections import deque

import numpy as np

import heightmap_ref as R
import heightmap_fill_ref as F

NO_VISIT = F.NO_VISIT
HVL_BASE, HVL_EXTENDED, HVL_INVALID = 0, 1, 2  # HeightmapVoxelLayer (ohmheightmap/HeightmapVoxel.h:17-28)
FILTERED = np.float32(-np.inf)  # kHeightmapVirtualSurfaceFilteredValue (private/HeightmapOperations.h:39-42)
MODE_UNORDERED, MODE_ORDERED = 2, 3
STATS = ("visits", "populated", "cells", "voxels", "repeats", "too_close", "filtered", "multi_layer_columns", "layers",
         "generations", "largest_generation")
# filterVirtualVoxels' 26 offsets: the count is of a set, their order does not matter
NEIGHBOURS = [(x, y, z) for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]


class _Slot:
    """One voxel of a heightmap column: what the three layers hold, and what L6 and source_visit need."""

    def __init__(self, occupancy, voxel, mean, visit, ground_key):
        self.occupancy, self.voxel, self.mean, self.visit, self.ground_key = occupancy, voxel, mean, visit, ground_key


class _Walk(F._Walk):
    """What both formulations share: L1 (F1 / F2), the column work of a visit (L2, L4), L3's test, L5, L6 and L7."""

    def __init__(self, src, p, mode, threshold):
        super().__init__(src, p)
        self.ordered = mode == MODE_ORDERED
        self.threshold = int(threshold) if self.ordered else 0
        self.min_clearance = p.min_clearance
        self.touched = {}   # grid cell -> heights touched, newest first (touched_grid_ / touched_list_)
        self.columns = {}   # heightmap cell (ca, cb) -> [_Slot]
        self.multi = set()  # multi_layer_keys
        self.by_ground = {}  # src_to_heightmap_keys: ground key -> (cell, the _Slot)
        self.log = []
        self.add_trace = []  # per add, stood or not: (visit, heightmap cell, voxels the column held)
        self.populated = self.repeats = self.too_close = self.filtered = 0
        # how often the walk met what the hand-made cases exist for (tests assert on these, the device has no such count)
        self.quirks = dict.fromkeys(("column_rule_refusals", "too_close_real", "permuted_columns", "base_not_nearest",
                                     "base_by_distance", "base_ties", "filtered_single", "filtered_multi"), 0)

    # L2, L4 and rule 5 up to the column
    def visit(self, ia, ib, h, seq):
        """(hg, candidate is null, the add or None)."""
        src, p = self.src, self.p
        a, b, up = self.a, self.b, self.up
        self.log.append((ia, ib, h))
        walk = self.key_of(ia, ib, h)
        candidate = R.supporting_voxel(src, walk, p.up_axis, self.min_key, self.max_key, self.voxel_floor,
                                       self.voxel_ceiling, self.clearance_permissive,
                                       self.first_flags if seq == 0 else self.flags)
        ground = R.find_ground(src, candidate, self.min_key, self.max_key, p.up_axis, self.up_vec, p, self.use_mean) \
            if candidate is not None else None
        ground_key = ground[0] if ground is not None else walk
        hg = ground_key[up] - self.min_key[up]
        base_candidate = ground is not None and (ground[1] > 0 or ground[2])  # L4, Heightmap.cpp:623-624
        voxel_type = src.occupancy_type(ground_key) if candidate is not None else R.K_NULL
        if not (voxel_type == R.K_OCCUPIED or (voxel_type == R.K_FREE and p.virtual_surface)):
            return hg, candidate is None, None
        pos = src.position(ground_key, self.use_mean) if voxel_type == R.K_OCCUPIED else src.centre(ground_key)
        src_height = R.dot(self.up_vec, pos)
        pos[up] = 0.0
        hk = self.hm.voxel_key(pos)
        assert hk is not None
        hr, hl = list(hk[0]), list(hk[1])
        hr[up], hl[up] = 0, 0
        ca = hr[a] * self.hm_dims[a] + hl[a] - self.first_cell[0]
        cb = hr[b] * self.hm_dims[b] + hl[b] - self.first_cell[1]
        assert 0 <= ca < self.ma and 0 <= cb < self.mb, (ca, cb, self.ma, self.mb)
        v = np.zeros((), dtype=R.HEIGHTMAP_VOXEL)
        v["clearance"] = np.float32(ground[1]) if ground is not None else np.float32(0.0)
        v["flags"] = R.HVF_OBSERVED_ABOVE if (ground is not None and ground[2]) else 0
        v["layer"] = HVL_BASE if base_candidate else HVL_EXTENDED
        if self.use_mean:
            m = src.mean(ground_key)
            v["contributing_samples"] = min(m[1], 0xFFFF) if m is not None else 0
        add = {"cell": (ca, cb), "hr": hr, "hl": hl, "src_height": src_height, "pos": pos, "voxel": v, "visit": seq,
               "occupancy": np.float32(1.0 if voxel_type == R.K_OCCUPIED else -1.0), "ground_key": tuple(ground_key)}
        return hg, candidate is None, add

    def slot_centre(self, hr, hl, slot):
        """voxelCentreGlobal of the cell's key moved `slot` steps along the raw up axis (regions one voxel high)."""
        region = list(hr)
        region[self.up] = slot
        return self.hm.voxel_centre(region, hl)

    def slot_height(self, add_or_cell, slot_index, slot):
        """double(float height) + dot(centre, up) of a voxel in slot `slot_index`."""
        return float(slot.voxel["height"]) + R.dot(self.slot_centre(add_or_cell[0], add_or_cell[1], slot_index),
                                                   self.up_vec)

    # L3
    def offer(self, cell, hg, null_candidate):
        """PlaneFillLayeredWalker::visit's test and touch: True when the offer is accepted."""
        heights = self.touched.setdefault(cell, [])
        if (len(heights) != 0) if null_candidate else (hg in heights):
            self.quirks["column_rule_refusals"] += null_candidate and hg not in heights
            return False
        heights.insert(0, hg)
        return True

    # L5
    def add(self, add):
        """addSurfaceVoxel (Heightmap.cpp:703-835) in a multi-layered mode."""
        column = self.columns.setdefault(add["cell"], [])
        self.add_trace.append((add["visit"], add["cell"], len(column)))
        key = (add["hr"], add["hl"])
        src_height = add["src_height"]
        if column:
            epsilon = 1e-3 * self.p.grid_resolution
            for k, slot in enumerate(column):  # haveRecordedHeight
                if abs(self.slot_height(key, k, slot) - src_height) < epsilon:
                    self.repeats += 1
                    return
            nearest_below = nearest_above = 0.0
            for k, slot in enumerate(column):  # :754-776
                delta = self.slot_height(key, k, slot) - src_height
                if delta < 0 and (nearest_below <= 0 or -delta < nearest_below):
                    nearest_below = -delta
                if delta > 0 and (nearest_above <= 0 or delta < nearest_above):
                    nearest_above = delta
            if (0 < nearest_below <= self.min_clearance) or (0 < nearest_above <= self.min_clearance):
                self.too_close += 1
                self.quirks["too_close_real"] += bool(add["occupancy"] > 0)
                return
            if self.ordered:
                self.multi.add(add["cell"])
        k = len(column)
        centre = self.slot_centre(add["hr"], add["hl"], k)
        v = add["voxel"].copy()
        v["height"] = np.float32(src_height - R.dot(centre, self.up_vec))  # relativeVoxelHeight
        mean = None
        if self.use_mean:  # DstVoxel::setPosition
            mean = (R.sub_voxel_coord([add["pos"][c] - centre[c] for c in range(3)], self.p.grid_resolution), 1)
        slot = _Slot(add["occupancy"], v, mean, add["visit"], add["ground_key"])
        column.append(slot)
        self.populated += 1
        if self.ordered and self.threshold > 0:
            self.by_ground.setdefault(add["ground_key"], (add["cell"], slot))  # emplace: the first entry stands

    # L6
    def filter_virtual(self):
        for ground_key, (cell, slot) in self.by_ground.items():
            if slot.occupancy != np.float32(-1.0):
                continue
            present = sum(tuple(ground_key[c] + n[c] for c in range(3)) in self.by_ground for n in NEIGHBOURS)
            if present < self.threshold:
                slot.voxel["layer"] = HVL_INVALID
                slot.occupancy = FILTERED
                self.filtered += 1
                self.quirks["filtered_multi" if cell in self.multi else "filtered_single"] += 1

    # L7
    def finalise(self):
        seed_height = R.dot(self.up_vec, list(self.p.reference_pos))
        for cell, column in self.columns.items():
            if not column:
                continue
            if cell not in self.multi:
                if column[0].voxel["layer"] == HVL_INVALID:
                    del column[:]
                else:
                    column[0].voxel["layer"] = HVL_BASE
                continue
            key = self.cell_key(cell)
            entries = []
            for order, slot in enumerate(column):
                invalid = slot.voxel["layer"] == HVL_INVALID
                height = float("inf") if invalid else \
                    R.dot(self.up_vec, self.slot_centre(key[0], key[1], order)) + float(slot.voxel["height"])
                entries.append((height, order, slot, slot.voxel["layer"] == HVL_BASE))
            if len(entries) <= 1:
                continue
            entries.sort(key=lambda e: (e[0], e[1]))
            self.quirks["permuted_columns"] += [e[1] for e in entries] != list(range(len(entries)))
            best = None  # (slot, clear above, absolute height)
            kept = []
            for at, (height, _, slot, base_candidate) in enumerate(entries):
                if slot.voxel["layer"] == HVL_INVALID:
                    continue  # sorted behind every valid voxel: its slot is cleared
                slot.voxel["height"] = np.float32(height - R.dot(self.up_vec, self.slot_centre(key[0], key[1], at)))
                if base_candidate:
                    clear = bool(slot.voxel["clearance"] > 0 or (slot.voxel["flags"] & R.HVF_OBSERVED_ABOVE))
                    # isOtherCandidateBetter (HeightmapOperations.cpp:135-165)
                    better = best is None or (not best[1] and clear) or \
                        (best[1] == clear and abs(height - seed_height) < abs(best[2] - seed_height))
                    if best is not None and best[1] == clear:
                        self.quirks["base_by_distance"] += better
                        self.quirks["base_ties"] += abs(height - seed_height) == abs(best[2] - seed_height)
                    if better:
                        best = (slot, clear, height)
                slot.voxel["layer"] = HVL_EXTENDED
                kept.append(slot)
            if best is not None:
                best[0].voxel["layer"] = HVL_BASE
                nearest = min(abs(e[0] - seed_height) for e in entries if e[2].voxel["layer"] != HVL_INVALID)
                self.quirks["base_not_nearest"] += abs(best[2] - seed_height) > nearest
            column[:] = kept

    def cell_key(self, cell):
        g = [0, 0, 0]
        g[self.a], g[self.b] = self.first_cell[0] + cell[0], self.first_cell[1] + cell[1]
        return ([g[c] // self.hm_dims[c] for c in range(3)], [g[c] % self.hm_dims[c] for c in range(3)])

    def finish(self, generation_sizes):
        res = self.res
        res.layers = max([len(c) for c in self.columns.values()] + [0])  # before removal
        if self.ordered:
            if self.threshold > 0:
                self.filter_virtual()
            self.finalise()
        slots = max(1, res.layers)
        res.slots = slots
        res.occupancy = np.full((slots, self.mb, self.ma), np.inf, dtype=np.float32)
        res.voxels = np.zeros((slots, self.mb, self.ma), dtype=R.HEIGHTMAP_VOXEL)
        res.mean = np.zeros((slots, self.mb, self.ma, 2), dtype=np.uint32) if self.use_mean else None
        res.source_visit = np.full((slots, self.mb, self.ma), NO_VISIT, dtype=np.uint32)
        res.layer_count = np.zeros((self.mb, self.ma), dtype=np.uint8)
        for (ca, cb), column in self.columns.items():
            res.layer_count[cb, ca] = len(column)
            for k, slot in enumerate(column):
                res.occupancy[k, cb, ca] = slot.occupancy
                res.voxels[k, cb, ca] = slot.voxel
                res.source_visit[k, cb, ca] = slot.visit
                if self.use_mean:
                    res.mean[k, cb, ca] = slot.mean
        res.log = np.array(self.log, dtype=np.uint32).reshape(-1, 3)
        res.visits = res.log.shape[0]
        res.populated, res.repeats, res.too_close, res.filtered = self.populated, self.repeats, self.too_close, self.filtered
        res.cells = int((res.layer_count != 0).sum())
        res.voxels_kept = int(res.layer_count.sum())
        res.multi_layer_columns = len(self.multi)
        res.generations = len(generation_sizes)
        res.largest_generation = max(generation_sizes)
        res.generation_sizes = list(generation_sizes)
        res.add_trace = list(self.add_trace)
        res.quirks = dict(self.quirks)
        return res


def stats_of(res):
    """The fields of ohmhip_heightmap_layered_stats in STATS order."""
    return (res.visits, res.populated, res.cells, res.voxels_kept, res.repeats, res.too_close, res.filtered,
            res.multi_layer_columns, res.layers, res.generations, res.largest_generation)


def _seed(w):
    return (w.seed[w.a] - w.min_key[w.a], w.seed[w.b] - w.min_key[w.b], w.seed[w.up] - w.min_key[w.up])


def build_layered(src, p, mode=MODE_ORDERED, threshold=0):
    """The reference as written.  None for an empty map / a null key, else a Result: occupancy, voxels, mean,
    source_visit as (slots, mb, ma) arrays, layer_count (mb, ma), log, and the stats of stats_of()."""
    w = _Walk(src, p, mode, threshold)
    if not w.ok or w.na <= 0 or w.nb <= 0:
        return None
    open_list = deque()
    key, generation = _seed(w), 0
    sizes = [0]
    seq = 0
    while True:
        ia, ib, h = key
        if len(sizes) <= generation:
            sizes.append(0)
        sizes[generation] += 1
        hg, null_candidate, add = w.visit(ia, ib, h, seq)
        seq += 1
        # onVisitWalker -> PlaneFillLayeredWalker::visit(ground_key, mode)
        for _, na, nb in w.neighbours(ia, ib):
            if w.offer(nb * w.na + na, hg, null_candidate):
                open_list.append(((na, nb, hg), generation + 1))
        if add is not None:
            w.add(add)
        if not open_list:
            break
        key, generation = open_list.popleft()
    return w.finish(sizes)


def build_layered_generations(src, p, mode=MODE_ORDERED, threshold=0):
    """The same result computed one generation at a time: every key's column work, then per grid cell the replay of
    the offers made to it in (key index) order, per heightmap cell the adds made to it in (key index) order; the
    accepted offers in (key index, neighbour slot) order are the next generation."""
    w = _Walk(src, p, mode, threshold)
    if not w.ok or w.na <= 0 or w.nb <= 0:
        return None
    items = [_seed(w)]
    seq = 0
    sizes = []
    while items:
        sizes.append(len(items))
        work = [w.visit(ia, ib, h, seq + i) for i, (ia, ib, h) in enumerate(items)]
        seq += len(items)
        offers, adds = {}, {}
        for i, (ia, ib, _) in enumerate(items):
            hg, null_candidate, add = work[i]
            for slot, na, nb in w.neighbours(ia, ib):
                offers.setdefault(nb * w.na + na, []).append((i, slot, hg, null_candidate))
            if add is not None:
                adds.setdefault(add["cell"], []).append((i, add))
        accepted = []
        for cell in sorted(offers):
            for i, slot, hg, null_candidate in sorted(offers[cell]):
                if w.offer(cell, hg, null_candidate):
                    accepted.append((i, slot, cell, hg))
        for cell in sorted(adds):
            for _, add in sorted(adds[cell], key=lambda e: e[0]):
                w.add(add)
        accepted.sort()
        items = [(cell % w.na, cell // w.na, hg) for _, _, cell, hg in accepted]
    return w.finish(sizes)
