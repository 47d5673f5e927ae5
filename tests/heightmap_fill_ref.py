"""CPU restatement of the flood-fill heightmap, ohm::Heightmap::buildHeightmap in HeightmapMode::kSimpleFill -- TEST
INFRASTRUCTURE.  The device fill (ohmhip_map_heightmap_fill) is held to it at exact equality: every cell, every field,
the visit log and the stats.

Written from the reference line by line (ohmheightmap/Heightmap.cpp:381-389, 522-700; PlaneFillWalker.cpp/.h); the rule
numbers F1-F6 are those of the fill block of include/ohmhip.h, rules 1, 3, 4 and 5 those of the heightmap block, taken
from tests/heightmap_ref.py.

build_fill()              the reference as written: one std::deque, one visit at a time
build_fill_generations()  the same walk one generation of the queue at a time, the cell events of a generation replayed
                          per cell in (key index, pop before offers, neighbour slot) order: the device formulation"""
from collections import deque

import numpy as np

import heightmap_ref as R

NO_VISIT = 0xFFFFFFFF


class _Walk:
    """What both formulations share: rules F1 / F2 and the column work of a visit (F3, F6)."""

    def __init__(self, src, p):
        self.src, self.p = src, p
        self.ext = R.extents(src, p)
        self.ok = self.ext is not None
        if not self.ok:
            return
        self.min_key, self.max_key = self.ext
        self.a, self.b, self.up = R.axis_indices(p.up_axis)
        self.up_vec = [0.0, 0.0, 0.0]
        self.up_vec[self.up] = 1.0 if p.up_axis >= 0 else -1.0
        self.use_mean = src.has_mean and not p.ignore_voxel_mean
        self.first_flags = (R.F_VIRTUAL if p.virtual_surface else 0) | \
            (R.F_PROMOTE_BELOW if p.promote_virtual_below else 0)
        self.flags = self.first_flags | R.F_BIAS_ABOVE  # Heightmap.cpp:385-386; kIgnoreVirtualAbove is never set
        self.voxel_floor = R.point_to_region_coord(p.floor, src.resolution)
        self.voxel_ceiling = R.point_to_region_coord(p.ceiling, src.resolution)
        self.clearance_permissive = max(1, R.point_to_region_coord(p.min_clearance, src.resolution) - 1)
        ref_key = src.om.voxel_key(p.reference_pos)
        if ref_key is None:
            self.ok = False
            return
        # F2: isBounded / clampToAxis (Heightmap.cpp:552-556), then PlaneFillWalker::begin's clampTo
        g = src.to_global(ref_key)
        self.seed = [min(max(g[c], self.min_key[c]), self.max_key[c]) for c in range(3)]
        self.na = self.max_key[self.a] - self.min_key[self.a] + 1
        self.nb = self.max_key[self.b] - self.min_key[self.b] + 1
        self.hm, self.hm_dims, self.first_cell, self.ma, self.mb = R.heightmap_geometry(src, p, self.ext)
        res = R.Result()
        res.min_ext, res.max_ext, res.na, res.nb = self.min_key, self.max_key, self.na, self.nb
        res.first_cell, res.ma, res.mb = self.first_cell, self.ma, self.mb
        res.occupancy = np.full((self.mb, self.ma), np.inf, dtype=np.float32)
        res.voxels = np.zeros((self.mb, self.ma), dtype=R.HEIGHTMAP_VOXEL)
        res.mean = np.zeros((self.mb, self.ma, 2), dtype=np.uint32) if self.use_mean else None
        res.source_visit = np.full((self.mb, self.ma), NO_VISIT, dtype=np.uint32)
        res.populated = 0
        res.log = []
        res.revisits = 0
        res.raising_pops = 0
        self.res = res

    def key_of(self, ia, ib, h):
        key = [0, 0, 0]
        key[self.a], key[self.b] = self.min_key[self.a] + ia, self.min_key[self.b] + ib
        key[self.up] = self.min_key[self.up] + h  # keyHeight: the raw key axis
        return key

    def visit(self, ia, ib, h, seq):
        """F3 and F6 of the visit numbered seq at (ia, ib, h); returns hg, the ground key's height offset."""
        src, p, res = self.src, self.p, self.res
        a, b, up = self.a, self.b, self.up
        res.log.append((ia, ib, h))
        walk = self.key_of(ia, ib, h)
        candidate = R.supporting_voxel(src, walk, p.up_axis, self.min_key, self.max_key, self.voxel_floor,
                                       self.voxel_ceiling, self.clearance_permissive,
                                       self.first_flags if seq == 0 else self.flags)
        ground = R.find_ground(src, candidate, self.min_key, self.max_key, p.up_axis, self.up_vec, p, self.use_mean) \
            if candidate is not None else None
        ground_key = ground[0] if ground is not None else walk
        hg = ground_key[up] - self.min_key[up]
        voxel_type = src.occupancy_type(ground_key) if candidate is not None else R.K_NULL  # Heightmap.cpp:637
        if not (voxel_type == R.K_OCCUPIED or (voxel_type == R.K_FREE and p.virtual_surface)):
            return hg
        pos = src.position(ground_key, self.use_mean) if voxel_type == R.K_OCCUPIED else src.centre(ground_key)
        # addSurfaceVoxel (:703-835), not multi-layered: the write overwrites
        src_height = R.dot(self.up_vec, pos)
        pos[up] = 0.0
        hk = self.hm.voxel_key(pos)
        assert hk is not None
        hr, hl = list(hk[0]), list(hk[1])
        hr[up], hl[up] = 0, 0
        centre = self.hm.voxel_centre(hr, hl)
        ca = hr[a] * self.hm_dims[a] + hl[a] - self.first_cell[0]
        cb = hr[b] * self.hm_dims[b] + hl[b] - self.first_cell[1]
        assert 0 <= ca < self.ma and 0 <= cb < self.mb, (ca, cb, self.ma, self.mb)
        res.populated += 1
        res.occupancy[cb, ca] = 1.0 if voxel_type == R.K_OCCUPIED else -1.0
        v = np.zeros((), dtype=R.HEIGHTMAP_VOXEL)
        v["height"] = np.float32(src_height - R.dot(centre, self.up_vec))
        v["clearance"] = np.float32(ground[1]) if ground is not None else np.float32(0.0)
        v["flags"] = R.HVF_OBSERVED_ABOVE if (ground is not None and ground[2]) else 0
        if self.use_mean:
            m = src.mean(ground_key)
            v["contributing_samples"] = min(m[1], 0xFFFF) if m is not None else 0
            res.mean[cb, ca, 0] = R.sub_voxel_coord([pos[c] - centre[c] for c in range(3)], p.grid_resolution)
            res.mean[cb, ca, 1] = 1
        res.voxels[cb, ca] = v
        res.source_visit[cb, ca] = seq
        return hg

    def neighbours(self, ia, ib):
        """F4: (slot, cell a, cell b) in the loop order of PlaneFillWalker::visit, cells off the grid skipped."""
        slot = 0
        for row_delta in (-1, 0, 1):
            for col_delta in (-1, 0, 1):
                if row_delta == 0 and col_delta == 0:
                    continue
                na, nb = ia + col_delta, ib + row_delta
                if 0 <= na < self.na and 0 <= nb < self.nb:
                    yield slot, na, nb
                slot += 1

    def finish(self, generation_sizes, max_multiplicity):
        res = self.res
        res.log = np.array(res.log, dtype=np.uint32).reshape(-1, 3)
        res.visits = res.log.shape[0]
        res.cells = int((res.source_visit != NO_VISIT).sum())
        res.generations = len(generation_sizes)
        res.largest_generation = max(generation_sizes)
        res.generation_sizes = list(generation_sizes)
        res.max_cell_multiplicity = max_multiplicity  # keys of one cell in one generation, the most
        return res


def _multiplicity(cells):
    counts = {}
    for c in cells:
        counts[c] = counts.get(c, 0) + 1
    return max(counts.values())


def build_fill(src, p):
    """The reference as written.  None for an empty map / a null key, else a Result: the dense arrays of
    heightmap_ref.build_heightmap with source_visit (sequence number of the visit that wrote the cell) in place of
    source_column; log (visits, 3) u32 ia, ib, h; visits, populated, cells, revisits (accepted offers to a cell that
    already held a height), generations, largest_generation; raising_pops, max_cell_multiplicity, generation_sizes."""
    w = _Walk(src, p)
    if not w.ok or w.na <= 0 or w.nb <= 0:
        return None
    res = w.res
    grid = [-1] * (w.na * w.nb)  # PlaneFillWalker::Visit::height
    open_list = deque()
    generation_of = deque()
    key = (w.seed[w.a] - w.min_key[w.a], w.seed[w.b] - w.min_key[w.b], w.seed[w.up] - w.min_key[w.up])
    generation = 0
    per_generation = [[]]
    seq = 0
    while True:
        ia, ib, h = key
        if len(per_generation) <= generation:
            per_generation.append([])
        per_generation[generation].append(ib * w.na + ia)
        hg = w.visit(ia, ib, h, seq)
        seq += 1
        # F4 onVisitWalker -> PlaneFillWalker::visit(ground_key): Revisit::kLower; the visiting cell is not touched
        for _, na, nb in w.neighbours(ia, ib):
            n = nb * w.na + na
            if grid[n] < 0 or hg < grid[n]:
                res.revisits += grid[n] >= 0
                open_list.append((na, nb, hg))
                generation_of.append(generation + 1)
                grid[n] = hg
        # F5 walkNext
        if not open_list:
            break
        key = open_list.popleft()
        generation = generation_of.popleft()
        cell = key[1] * w.na + key[0]
        res.raising_pops += key[2] > grid[cell]
        grid[cell] = key[2]
    return w.finish([len(g) for g in per_generation], max(_multiplicity(g) for g in per_generation))


def build_fill_generations(src, p):
    """The same result computed one generation at a time: first every key's column work, then per touched cell the
    replay of its events -- the pop of key i at the cell, the offer of key i through neighbour slot k -- in (i, pop
    before offers, k) order; the accepted offers in (i, k) order are the next generation."""
    w = _Walk(src, p)
    if not w.ok or w.na <= 0 or w.nb <= 0:
        return None
    res = w.res
    grid = [-1] * (w.na * w.nb)
    items = [(w.seed[w.a] - w.min_key[w.a], w.seed[w.b] - w.min_key[w.b], w.seed[w.up] - w.min_key[w.up])]
    seq = 0
    sizes = []
    multiplicity = 0
    first = True
    while items:
        sizes.append(len(items))
        multiplicity = max(multiplicity, _multiplicity([ib * w.na + ia for ia, ib, _ in items]))
        # column step: independent per key
        hgs = [w.visit(ia, ib, h, seq + i) for i, (ia, ib, h) in enumerate(items)]
        seq += len(items)
        # cell step: the events, bucketed per cell (an item adds at most one event to a cell, so i orders them)
        events = {}
        for i, (ia, ib, h) in enumerate(items):
            if not first:  # the seed is never popped
                events.setdefault(ib * w.na + ia, []).append((i, -1, h))
            for slot, na, nb in w.neighbours(ia, ib):
                events.setdefault(nb * w.na + na, []).append((i, slot, hgs[i]))
        accepted = []
        for cell, evs in events.items():
            evs.sort()
            value = grid[cell]
            for i, slot, height in evs:
                if slot < 0:
                    res.raising_pops += height > value
                    value = height
                elif value < 0 or height < value:
                    res.revisits += value >= 0
                    accepted.append((i, slot, cell, height))
                    value = height
            grid[cell] = value
        accepted.sort()
        items = [(cell % w.na, cell // w.na, height) for _, _, cell, height in accepted]
        first = False
    return w.finish(sizes, multiplicity)
