"""Matrices past 65 536 rows and 65 536 aggregates for the graph set-ups -- the colouring and the colour-major permutation
(include/spmv_hip_mcgs.h), the two aggregations, the plan, the Galerkin product, the restrictions and the prolongation
(include/spmv_hip_agg.h, spmv_hip_agg_mis2.h) -- and what the restatements of mcgs_cases.py, agg_cases.py and agg_mis2_cases.py make
of them, once per process (test_graph_size_cases.py holds every figure quoted here, and the restated Galerkin product to sums formed
another way, without a device; test_gpu_graph_sizes.py holds the GPU to the restatements bit for bit on these matrices).

Three mechanisms of the set-up code change at these sizes and at no smaller one:

1. mcgs_chunk_scan_kernel (mcgs_kernels.hpp) is one wave over the sums of chunks of 1024 rows: 64 chunks a trip, the sum of a trip
   carried into the next.  Up to 65 536 rows there is one trip and no carry.  mcgs_offsets_kernel walks every chunk per lane.
2. The Galerkin sort key (agg_key_kernel, agg.hip) is agg[row] aggregates + agg[column] in 64 bits, sorted over bits_of(aggregates^2)
   bits and taken apart again by / and %: up to 65 536 aggregates that is at most 32 bits, from 65 537 on the upper word of the key
   is used, the radix sort makes further passes and the divisions are of keys that no unsigned holds.
3. Everything sized by the rows in workgroups of 256: the per-wave counters of the rounds, the prefix sums over rows + 1 and
   nnz + 1, the plan's sort over bits_of(aggregates) bits, the counts per aggregate.

| case                       | rows              | why                                                                                     |
| path_65536, path_65537     | 65 536 / 65 537   | 64 chunks against 65: the last size of one trip, and the first carry (one live lane)     |
| grid_300x300               | 90 000            | 88 chunks (a second trip of 24 lanes); 32 846 distance-1 aggregates: a key of 31 bits,   |
|                            |                   | the control below the edge of 32                                                        |
| path_200001                | 200 001           | 196 chunks (four trips, the last of 4 lanes); 86 450 distance-1 aggregates (33 bits);   |
|                            |                   | 54 967 distance-2 aggregates                                                            |
| grid_512x512               | 262 144           | 256 chunks (four full trips); 95 432 distance-1 aggregates, 30 877 of them single rows;  |
|                            |                   | 560 366 coarse entries; a key of 34 bits                                                |
| blocks_65536, blocks_65537 | 98 304 / 98 305   | mc.path(n) under the hand-made plan ac.blocks(n, 2): exactly 65 536 aggregates (a key   |
|                            |                   | of 32 bits, the plan's sort over 16) against 65 537 (33 and 17): the edge, either side   |

The figures are those of the restatements at seed ac.SEEDS[0], theta 0 (FIGURES, HIERARCHY below; asserted in
test_graph_size_cases.py): a case whose figure moved no longer reaches its edge and is chosen anew, not recorded anew."""
import functools

import numpy as np

import agg_cases as ac
import agg_mis2_cases as a2
import mcgs_cases as mc

CHUNK = 1024  # kMcgsChunk: rows per wave in the counting sort and the scan
WAVE = 64

GENERATORS = {
    "path_65536": lambda: mc.path(65536),
    "path_65537": lambda: mc.path(65537),
    "grid_300x300": lambda: mc.grid(300, 300),
    "path_200001": lambda: mc.path(200001),
    "grid_512x512": lambda: mc.grid(512, 512),
}
MATRICES = tuple(GENERATORS)
BLOCKS = {"blocks_65536": 98304, "blocks_65537": 98305}  # rows of the path under ac.blocks(rows, 2)
BOTH_SEEDS = ("path_65536", "path_65537")               # the colouring runs under both seeds here, under the first elsewhere
SWEEPS = ("path_65537", "grid_300x300")
DISTANCE_2 = ("path_200001", "grid_512x512")
GALERKIN = ("grid_300x300", "path_200001", "grid_512x512")
SEED = ac.SEEDS[0]

# name -> (rows, chunks, lanes of the chunk scan's last trip, trips)
CHUNKS = {
    "path_65536": (65536, 64, 64, 1),
    "path_65537": (65537, 65, 1, 2),
    "grid_300x300": (90000, 88, 24, 2),
    "path_200001": (200001, 196, 4, 4),
    "grid_512x512": (262144, 256, 64, 4),
}
# name -> the status [aggregates, rounds, largest, singletons] is not quoted beyond what the reasons above need:
# (distance-1 aggregates, bits of the Galerkin key, bits of the plan's sort)
FIGURES = {
    "grid_300x300": (32846, 31, 16),
    "path_200001": (86450, 33, 17),
    "grid_512x512": (95432, 34, 17),
    "blocks_65536": (65536, 32, 16),
    "blocks_65537": (65537, 33, 17),
}
DISTANCE_2_AGGREGATES = {"path_200001": 54967}
# the distance-1 hierarchy of grid_512x512, each level on the coarse arrays of the one before:
# (rows, status [aggregates, rounds, largest, singletons], coarse entries, bits of the key, the longest run)
HIERARCHY = (
    (262144, [95432, 5, 5, 30877], 560366, 34, 13),
    (95432, [33350, 5, 9, 12643], 206062, 31, 41),
    (33350, [12996, 5, 15, 6514], 75784, 28, 73),
    (12996, [6366, 4, 19, 4062], 33292, 26, 87),
)


def bits_of(keys):
    """agg.hip's bits_of: the bits that hold every key below `keys`, at least one."""
    bits = 1
    while bits < 64 and (1 << bits) < keys:
        bits += 1
    return bits


def chunks_of(rows):
    """(chunks of 1024 rows, the live lanes of the chunk scan's last trip, its trips)."""
    chunks = -(-rows // CHUNK)
    return chunks, (chunks - 1) % WAVE + 1, -(-chunks // WAVE)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(rows, row_ptr, columns, values); a blocks_* case is the path its plan lies over."""
    return mc.path(BLOCKS[name]) if name in BLOCKS else GENERATORS[name]()


@functools.lru_cache(maxsize=None)
def general_values(name):
    """agg_cases.general_values on these matrices: doubles that no float holds, seeded by the name."""
    return np.random.default_rng(len(name) + 41).uniform(-1.0, 1.0, size=len(matrix(name)[2]))


@functools.lru_cache(maxsize=None)
def distinct_values(name):
    """The matrix's own values, each stretched by its own factor in [1, 1.25): no two entries of a row alike, so a copy from
    another row or entry shows, and the diagonal still as large as a sweep wants it."""
    v = matrix(name)[3]
    return v * (1.0 + 0.25 * np.random.default_rng(len(name) + 43).uniform(0.0, 1.0, size=len(v)))


# ---- the colouring and its plan ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def colouring(name, seed=SEED):
    """(mc.Plan over distinct_values(name), colours, status)."""
    rows, p, c, _ = matrix(name)
    col_of, status = mc.colour(rows, p, c, seed)
    return mc.Plan(rows, p, c, distinct_values(name), col_of, status), col_of, status


# ---- the aggregates, their plans and products -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def aggregates(name, distance=1, theta=0.0):
    """(agg, status) of the first seed; at a theta above 0 over general_values(name), which the thresholds then read."""
    rows, p, c, v = matrix(name)
    values = general_values(name) if theta > 0.0 else v
    return (ac.aggregate if distance == 1 else a2.aggregate)(rows, p, c, values, theta, SEED)


@functools.lru_cache(maxsize=None)
def plan(name, distance=1):
    """ac.Plan: of the restated aggregates, or the hand-made ac.blocks(rows, 2) of a blocks_* case."""
    if name in BLOCKS:
        return ac.blocks(BLOCKS[name], 2)
    agg, status = aggregates(name, distance)
    return ac.Plan(matrix(name)[0], agg, status)


@functools.lru_cache(maxsize=None)
def coarse(name):
    """ac.Coarse of the distance-1 plan (the hand-made one of a blocks_* case)."""
    rows, p, c, _ = matrix(name)
    return ac.Coarse(plan(name), p, c)


@functools.lru_cache(maxsize=None)
def coarse_values(name):
    return coarse(name).values(general_values(name))


class Level:
    """One level of the hierarchy as the restatements give it: the matrix, its aggregates, plan, product and coarse values."""

    def __init__(self, rows, p, c, v):
        self.rows, self.p, self.c, self.v = rows, p, c, v
        self.agg, self.status = ac.aggregate(rows, p, c, v, 0.0, SEED)
        self.plan = ac.Plan(rows, self.agg, self.status)
        self.coarse = ac.Coarse(self.plan, p, c)
        self.cv = self.coarse.values(v)
        self.key_bits = bits_of(self.plan.aggregates ** 2)
        self.longest = int(np.diff(self.coarse.entry_ptr).max())

    def next(self):
        return Level(self.plan.aggregates, self.coarse.row_ptr, self.coarse.column, self.cv)


@functools.lru_cache(maxsize=None)
def hierarchy():
    """The four distance-1 levels of grid_512x512 over general_values: each level's matrix is the coarse pattern and the coarse
    values of the one before (at theta 0 no aggregate depends on a value: the figures are those of the grid's own values)."""
    rows, p, c, _ = matrix("grid_512x512")
    levels = [Level(rows, p, c, general_values("grid_512x512"))]
    while len(levels) < len(HIERARCHY):
        levels.append(levels[-1].next())
    return tuple(levels)
