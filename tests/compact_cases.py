"""What test_compact_capi.py and test_gpu_compact.py share: the matrices, and the encoding of include/spmv_hip_compact.h restated
in numpy (window bases chosen greedily from a tile's distinct columns, the compact / wide decision, the codes, every number of
plan_info) from nothing but row_ptr, the columns and the first four fields of the tile table."""
import functools

import numpy as np

import helpers
import oracle_py
from spmv_amd import capi, hostapi, synth

TILE, TILE_ROWS, WINDOWS, SPAN = 512, 64, 8, 8192


def _i32(*arrays):
    return tuple(np.ascontiguousarray(a, dtype=np.int32) for a in arrays)


def _csr(rows, cols, p, c, v):
    p, c = _i32(p, c)
    return int(rows), int(cols), p, c, np.ascontiguousarray(v, dtype=np.float64)


def from_lengths(lens, cols, seed, pick=None):
    """Rows of the given lengths with distinct sorted random columns (pick(rng, n): the columns of a row of n entries)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    p = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=p[1:])
    pick = pick or (lambda rng, n: rng.choice(cols, size=n, replace=False))
    c = np.concatenate([np.sort(pick(rng, int(n))) for n in lens] + [np.zeros(0, dtype=np.int64)])
    return _csr(len(lens), cols, p, c, rng.uniform(-1.0, 1.0, size=len(c)))


def from_rows(rows_of_columns, cols, seed=1):
    lens = [len(r) for r in rows_of_columns]
    p = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=p[1:])
    c = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows_of_columns] + [np.zeros(0, dtype=np.int64)])
    return _csr(len(lens), cols, p, c, np.random.default_rng(seed).uniform(-1.0, 1.0, size=len(c)))


def _load(spec):
    A = hostapi.load(spec, "csr")
    out = _csr(A.rows, A.cols, np.array(A.row_ptr), np.array(A.column_index), np.array(A.value))
    A.close()
    return out


def windows_tile(nwindows, cols=None, per_window=40, rows=8):
    """One tile of `rows` equal rows whose columns need exactly `nwindows` windows: window w holds per_window columns from
    w * (SPAN + 5), each row takes every rows-th of them."""
    allc = np.concatenate([w * (SPAN + 5) + np.arange(per_window) * 3 for w in range(nwindows)])
    cols = cols or int(allc.max()) + 1
    return from_rows([np.sort(allc[r::rows]) for r in range(rows)], cols)


def edge_columns():
    """Columns at cols - 1, at multiples of 8192 and one below them; cols itself is a multiple of 8192 plus one."""
    cols = 5 * SPAN + 1
    marks = np.unique(np.concatenate([np.arange(0, cols, SPAN), np.arange(SPAN, cols, SPAN) - 1, [cols - 1, cols - 2, 1]]))
    rows = [marks, marks[::2], marks[1::2], [cols - 1], [0, cols - 1], [SPAN - 1, SPAN, 2 * SPAN - 1, 2 * SPAN, 2 * SPAN + 8191, cols - 1]]
    rows += [np.sort(np.random.default_rng(s).choice(cols, size=9, replace=False)) for s in range(40)]
    return from_rows(rows, cols)


def mixed_mesh_and_graph():
    """A 3-D mesh block (compact tiles) stacked on power-law rows over the same columns (wide tiles): both branches of the
    kernel in one launch."""
    mr, mc, mp, mj, mv = _csr(*synth.delaunay_mesh(30000, 1, seed=5, order="rcm"))
    gr, gc, gp, gj, gv = _csr(*synth.powerlaw(40000, 2_000_000, seed=6, max_len=3000)[:5])
    cols = max(mc, gc)
    p = np.concatenate([mp, mp[-1] + gp[1:]])
    return _csr(mr + gr, cols, p, np.concatenate([mj, gj]), np.concatenate([mv, gv]))


def _golden():
    g = helpers.load_golden()
    oracle = oracle_py.Oracle()
    out = {}
    for case in g["cases"]:
        rows, cols, i, j, a, _, _ = helpers.parse_mtx_text(helpers.case_mtx(g, case))
        p, c, v = oracle.csr_from_coordinate(rows, i, j, a, row_alignment=1)
        out["golden_" + case["name"]] = lambda rows=rows, cols=cols, p=p, c=c, v=v: _csr(rows, cols, p, c, v)
    assert out
    return out


def _empty_rows():
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 7, size=30000)
    lens[::7] = 0
    lens[5000:9000] = 0
    return from_lengths(lens, 20000, 4)


def _dense_row(cols, near):
    lens = np.random.default_rng(8).integers(0, 4, size=3000)
    lens[1717] = 9000
    # near: the dense row's columns within three windows; otherwise spread over `cols` (more than eight windows: a wide long row)
    pick = (lambda rng, n: rng.choice(min(cols, 3 * SPAN) if n > 100 and near else cols, size=n, replace=False))
    return from_lengths(lens, cols, 9, pick)


CASES = {
    "poisson_512": lambda: _csr(*synth.poisson2d(512)[:5]),
    "delaunay_60k_1dof_rcm": lambda: _csr(*synth.delaunay_mesh(60000, 1, seed=3, order="rcm")),
    "delaunay_60k_3dof_rcm": lambda: _csr(*synth.delaunay_mesh(60000, 3, seed=3, order="rcm")),
    "kkt_60": lambda: _load("synthetic:kkt:60"),
    "queen_40_32_24": lambda: _load("synthetic:queen:40,32,24"),
    "powerlaw_graph": lambda: _csr(*synth.powerlaw(200000, 200000, seed=4)[:5]),
    "banded": lambda: _csr(*synth.banded(50000, [-40, -3, -1, 0, 1, 2, 57])[:5]),
    "banded_five_windows": lambda: _csr(*synth.banded(100000, [-30000, -9000, 0, 9000, 30000])[:5]),
    "empty_rows": _empty_rows,
    "dense_row_9000_compact": lambda: _dense_row(20000, True),
    "dense_row_9000_wide": lambda: _dense_row(400000, False),
    "rows_0_to_7_ragged_end": lambda: from_lengths(np.append(np.random.default_rng(13).integers(0, 8, size=10006), 5), 9001, 14),
    "eight_windows": lambda: windows_tile(8),
    "nine_windows": lambda: windows_tile(9),
    "edge_columns": edge_columns,
    "mixed_mesh_and_graph": mixed_mesh_and_graph,
    "one_by_one": lambda: _csr(1, 1, [0, 1], [0], [2.5]),
    "no_rows": lambda: _csr(0, 7, [0], [], []),
    "no_cols": lambda: _csr(7, 0, np.zeros(8), [], []),
    "no_entries": lambda: _csr(10, 12, np.zeros(11), [], []),
}
CASES.update(_golden())
NAMES = sorted(CASES)


@functools.lru_cache(maxsize=3)
def matrix(name):
    return CASES[name]()


# ---- the encoding, restated ---------------------------------------------------------------------------------------------------------

def greedy_bases(columns):
    """(windows needed, base[8] or None when more than eight are needed) for the columns of one tile."""
    u = np.unique(columns)
    if len(u) == 0:
        return 1, np.zeros(WINDOWS, dtype=np.int64)  # a tile without entries: compact, one window, bases 0
    bases = [int(u[0])]
    while True:
        i = int(np.searchsorted(u, bases[-1] + SPAN, side="left"))  # the smallest column >= base + 8192
        if i == len(u):
            break
        bases.append(int(u[i]))
    if len(bases) > WINDOWS:
        return len(bases), None
    return len(bases), np.array(bases + [bases[-1]] * (WINDOWS - len(bases)), dtype=np.int64)


def recount(rows, cols, p, c, flags, info, tab, codes):
    """Every claim of spmv_hip_c16_plan_preview recounted from row_ptr, the columns and the first four fields of its table."""
    p = p.astype(np.int64)
    c = c.astype(np.int64)
    nnz = int(p[rows])
    assert info["rows"] == rows and info["cols"] == cols and info["stored_entries"] == nnz and info["flags"] == flags
    if rows == 0 or cols == 0 or nnz == 0:  # the multiply does nothing
        assert tab.shape == (0, capi.C16_TILE_INTS)
        assert all(v == 0 for k, v in info.items() if k not in ("rows", "cols", "stored_entries", "flags")), info
        return
    nt = info["tiles"]
    assert tab.shape == (nt, capi.C16_TILE_INTS) and nt > 0 and len(codes) == nnz
    r0, k0, nr = (tab[:, i].astype(np.int64) for i in range(3))
    k1 = p[r0 + nr]
    kb = k0 & ~3
    lens = np.diff(p)
    long_tiles = (nr == 1) & (k1 - kb > TILE)
    compact = wide = centries = quads = row_ptr_bytes = 0
    hist = [0] * WINDOWS
    want_codes = np.zeros(nnz, dtype=np.int64)
    for w in range(nt):
        cw = c[k0[w]:k1[w]]
        need, bases = greedy_bases(cw)
        if bases is None:
            assert need > WINDOWS and tab[w, 4] == 0 and not np.any(tab[w, 5:]), (w, need, tab[w])
            wide += 1
        else:
            assert tab[w, 4] == need and np.array_equal(tab[w, 5:], bases), (w, need, bases, tab[w])
            compact += 1
            hist[need - 1] += 1
            centries += len(cw)
            if len(cw):
                win = np.searchsorted(bases[:need], cw, side="right") - 1
                off = cw - bases[win]
                assert np.all((win >= 0) & (off >= 0) & (off < SPAN))
                want_codes[k0[w]:k1[w]] = (win << 13) | off
                quads += (k1[w] - 1 - kb[w]) // 4 + 1
            # what the kernel computes from the codes the library returned
            got = codes[k0[w]:k1[w]].astype(np.int64)
            assert np.array_equal(tab[w, 5:].astype(np.int64)[got >> 13] + (got & 0x1FFF), cw), (w, "decode")
        if not long_tiles[w]:
            tl = lens[r0[w]:r0[w] + nr[w]]
            fast = k1[w] > k0[w] and ((k1[w] - 1) & ~3) + 4 <= nnz
            if not (fast and tl.min() == tl.max()):
                row_ptr_bytes += 4 * (int(nr[w]) + 1)
    assert np.array_equal(codes.astype(np.int64), want_codes)
    assert info["compact_tiles"] == compact and info["wide_tiles"] == wide and compact + wide == nt
    assert info["long_row_tiles"] == int(long_tiles.sum()) and info["compact_entries"] == centries
    assert [info["tiles_with_%d_windows" % (i + 1)] for i in range(WINDOWS)] == hist
    assert info["workgroups"] == -(-nt // 4)
    assert info["device_bytes"] == -(-(16 * (nt + 1) + 32 * nt + 8 * quads) // 16) * 16
    assert info["streamed_bytes"] == 6 * centries + 8 * (nnz - centries) + row_ptr_bytes + 16 * rows + 8 * cols + 16 * (nt + 1) + 32 * nt
