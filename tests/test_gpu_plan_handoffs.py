"""Repack's hand-offs from windows to tiles (plan_csr.hip, repack_stages): when block tiles, group tiles or masked stencil tiles take
most of the tiles, the plan gives up the block windows (csr_clear_blockwin_kernel) or the segment windows (csr_clear_segwin_kernel)
that compress built, and a value dictionary asked for earlier is asked for again.  Every case first proves through plan_info that it
reached its hand-off -- without the tile stage (FLAG_NO_BLOCK_TILES, or FLAG_NO_SHIFTED_TILES for the grid) the windows are there,
with it they are gone (majority) or kept (minority) -- then checks the whole y against the oracle, its variants and the context's
upload.  (The review's natural case, a 2-dof Delaunay mesh in RCM order with 300 K nodes, gets no segment windows: it does not
reach the hand-off and is not here.)  Round 6's review: a NARROW group tile inside a claimed segment-window block lost kTileMetaNarrow with the windows and was
then read as a WIDE group tile (its window slots taken for 32-bit columns): y silently wrong, no fault."""
import numpy as np
import pytest

from helpers import assert_close, abs_products
from spmv_amd import capi, synth

pytestmark = pytest.mark.gpu


def band_mesh(nodes, d, k, w, far_every=0, far_nodes=2, far_share=0.75, broken=0.0, levels=0, seed=1, alt=False):
    """A mesh with `d` unknowns per node, numbered node by node (the d rows of a node share their columns: dense d x d blocks): node
    i is coupled to itself and k - 1 random nodes within +-w -- every row d * k entries long, so tiles hold whole nodes whether the
    plan cuts them on groups or not.  In the first `far_share` of the nodes a band of `far_nodes` nodes every `far_every` swaps one
    of its couplings for a node more than 65 536 columns away: their tiles are wide, and a block of 32 tiles holding one of them
    mixes narrow and wide tiles.  `broken`: that share of the nodes gets a foreign column (last entry + 1) in its second row.
    `levels` > 0: values from a dictionary of that many.  `alt`: odd nodes get k + 1 couplings (rows of two lengths: with d = 2 the
    row lengths alone say groups of 2, not 4)."""
    rng = np.random.default_rng(seed)
    far = -(-70000 // d)  # nodes: more than 65 536 columns
    assert nodes >= 2 * far and k <= 2 * w + 1  # (every node has a node that far away)
    i = np.arange(nodes)
    lo = np.clip(i - w, 0, nodes - 2 * w - 1)
    score = rng.random((nodes, 2 * w + 1))
    score[i, i - lo] = -1.0  # the diagonal is always chosen
    nbr = lo[:, None] + np.argpartition(score, k - 1, axis=1)[:, :k]
    nbr.sort(axis=1)
    if far_every:
        band = (i % far_every < far_nodes) & (i < far_share * nodes)
        b = i[band]
        other = np.where(nbr[b, 0] == b, 1, 0)  # a coupling that is not the diagonal
        nbr[b, other] = np.where(b + far < nodes, b + far, b - far)
        nbr.sort(axis=1)
    rows, n = nodes * d, k * d
    c = np.repeat(((nbr * d)[:, :, None] + np.arange(d)).reshape(nodes, 1, n), d, axis=1).reshape(rows, n)
    keep = np.ones((rows, n), dtype=bool)
    if alt:  # even nodes lose their first coupling that is neither the diagonal nor far away
        even = i[i % 2 == 0]
        local = (nbr[even] != even[:, None]) & (np.abs(nbr[even] - even[:, None]) <= w)
        keep.reshape(nodes, d, k, d)[even, :, np.argmax(local, axis=1), :] = False
    if broken > 0:
        hit = i[rng.random(nodes) < broken] * d + 1
        hit = hit[c[hit, -1] + 1 < rows]
        c[hit, -1] += 1
    p = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=p[1:])
    c = c[keep]
    if levels:
        v = rng.choice(rng.uniform(-1.0, 1.0, size=levels), size=len(c))
    else:
        v = rng.uniform(-1.0, 1.0, size=len(c))
    return rows, rows, p.astype(np.int32), c.astype(np.int32), v


def run_plan(rows, cols, p, c, v, x, y0, flags=0, runs=1, other_columns=False, out_of_place=False, index_values=None):
    """index_values: None, "after" (compress, repack, index_values) or "before" (compress, index_values, repack)."""
    import torch
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    tp, tc, tv, tx = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (p, c, v, x))
    plan = capi.CsrPlan(rows, cols, p, capi.CSR_AUTO, 0, flags)
    plan.compress(tc.data_ptr(), stream)
    if index_values == "before":
        plan.index_values(tv.data_ptr(), stream)
    plan.repack(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), stream)
    if index_values == "after":
        plan.index_values(tv.data_ptr(), stream)
    info = plan.info()
    cols_now = tc.clone() if other_columns else tc
    ty = torch.from_numpy(y0.copy()).to(dev)
    if out_of_place:
        tout = torch.full((rows,), np.nan, dtype=torch.float64, device=dev)
        plan.spmv_out(tp.data_ptr(), cols_now.data_ptr(), tv.data_ptr(), tx.data_ptr(), ty.data_ptr(), tout.data_ptr(), stream)
        ty = tout
    else:
        for _ in range(runs):
            plan.spmv(tp.data_ptr(), cols_now.data_ptr(), tv.data_ptr(), tx.data_ptr(), ty.data_ptr(), stream)
    torch.cuda.synchronize()
    got = ty.cpu().numpy()
    plan.close()
    return got, info


def same_bits(a, b, what):
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)), what


def short(info):
    keys = ("row_blocks", "narrow_tiles", "segwin_tiles", "blockwin_tiles", "group_rows", "group_tiles", "block_tiles",
            "masked_block_tiles", "shifted_tiles", "stencil_mask_tiles", "indexed_values", "streamed_bytes")
    return {k: info[k] for k in keys}


def check_y(oracle, what, rows, cols, p, c, v, index_values=None, nterms=None, other_columns_bits=True):
    """The whole y and its variants; returns the default plan's info."""
    x = synth.x_vector(cols, seed=3)
    y0 = synth.x_vector(rows, seed=4)
    nterms = nterms or int(np.max(np.diff(p))) + 1
    want = oracle.csr_spmv(rows, p, c, v, x, y=y0, num_threads=4)
    scale = abs_products(rows, p, c, v, x) + np.abs(y0)
    got, info = run_plan(rows, cols, p, c, v, x, y0, index_values=index_values)
    assert_close(got, want, scale, what=what, nterms=nterms)
    got3, _ = run_plan(rows, cols, p, c, v, x, y0, runs=3, index_values=index_values)
    assert_close(got3, oracle.csr_spmv(rows, p, c, v, x, y=y0, num_threads=4, runs=3), 3 * scale, what=what + ", three runs", nterms=3 * nterms)
    got_o, _ = run_plan(rows, cols, p, c, v, x, y0, out_of_place=True, index_values=index_values)
    same_bits(got_o, got, what + ", y_out")
    got_c, _ = run_plan(rows, cols, p, c, v, x, y0, other_columns=True, index_values=index_values)
    if other_columns_bits:
        same_bits(got_c, got, what + ", other column array")
    else:  # (block tiles: nothing derived from the plan's columns may be used, so another summation order -- test_gpu_blocktiles.py)
        assert_close(got_c, want, scale, what=what + ", other column array", nterms=nterms)
    got_e, _ = run_plan(rows, cols, p, c, v, x, y0, flags=capi.FLAG_EXACT_ORDER, index_values=index_values)
    same_bits(got_e, oracle.csr_spmv(rows, p, c, v, x, y=y0, num_threads=1), what + ", exact order")
    for flag, name in ((capi.FLAG_NO_SEGMENT_WINDOW, "no segment windows"), (capi.FLAG_NO_BLOCK_TILES, "no block tiles")):
        got_f, _ = run_plan(rows, cols, p, c, v, x, y0, flags=flag, index_values=index_values)
        assert_close(got_f, want, scale, what=what + ", " + name, nterms=nterms)
    with capi.Context(0) as ctx:
        ctx.upload_csr(rows, cols, p, c, v)
        ctx.set_x(x)
        ctx.run()
        assert_close(ctx.get_y(), oracle.csr_spmv(rows, p, c, v, x, num_threads=4), abs_products(rows, p, c, v, x),
                     what=what + ", csr upload", nterms=nterms)
    return info


def plan_info(rows, cols, p, c, v, flags=0, index_values=None):
    x = np.zeros(cols)
    return run_plan(rows, cols, p, c, v, x, np.zeros(rows), flags=flags, index_values=index_values)[1]


def tiles_of(info, d):
    return info["group_tiles"] if d in (2, 4) else info["block_tiles"]


# (d, k, w): every row d * k entries (d = 2: 40 or 42), tiles of whole nodes with and without the group cut (12 rows / 8 rows of 60 /
# 6 rows of 84)
MESHES = {2: (72000, 21, 150), 4: (36000, 15, 150), 3: (48000, 28, 150), 6: (24000, 14, 150)}
# a band of 2 nodes with a far coupling every so many nodes: fewer than the nodes of a 32-tile block
FAR_EVERY = {2: 150, 4: 50, 3: 50, 6: 25}


def mesh_case(d, broken=0.0, levels=0, far_share=0.75):
    nodes, k, w = MESHES[d]
    return band_mesh(nodes, d, k, w, far_every=FAR_EVERY[d], far_share=far_share, broken=broken, levels=levels, seed=10 + d, alt=d == 2)


def assert_segment_windows_first(info_n, what):
    assert info_n["segwin_tiles"] > 0 and 0 < info_n["narrow_tiles"] < info_n["row_blocks"], (what, short(info_n))


@pytest.mark.parametrize("d", [2, 4, 3, 6])
def test_segment_windows_given_up_for_a_tile_majority(oracle, d):
    """(a) / (c): segment windows claim the blocks that mix narrow and wide tiles; then group tiles (d = 2, 4) or block tiles
    (d = 3, 6) take most of the tiles, claimed narrow ones included, and the windows are dropped."""
    what = "%d unknowns per node, segment windows then a tile majority" % d
    rows, cols, p, c, v = mesh_case(d)
    assert_segment_windows_first(plan_info(rows, cols, p, c, v, flags=capi.FLAG_NO_BLOCK_TILES), what)
    info = check_y(oracle, what, rows, cols, p, c, v, other_columns_bits=d in (2, 4))
    assert tiles_of(info, d) > info["row_blocks"] / 2 and info["segwin_tiles"] == 0 and info["blockwin_tiles"] == 0, (what, short(info))


def test_segment_windows_given_up_under_a_value_dictionary(oracle):
    """(a) with values from a dictionary of 100: the dictionary launch multiplies the claimed narrow tiles that lost their windows
    (no group tiles under it): they must read their 32-bit columns, not the window slots left in their 16-bit stream."""
    what = "4 unknowns per node, dictionary"
    rows, cols, p, c, v = mesh_case(4, levels=100)
    assert_segment_windows_first(plan_info(rows, cols, p, c, v, flags=capi.FLAG_NO_BLOCK_TILES), what)
    for order in ("after", "before"):
        info = check_y(oracle, what + ", index_values " + order, rows, cols, p, c, v, index_values=order)
        assert info["indexed_values"] == 100 and info["segwin_tiles"] == 0 and info["blockwin_tiles"] == 0, (what, order, short(info))


@pytest.mark.parametrize("d", [2, 4])
def test_segment_windows_kept_beside_a_group_minority(oracle, d):
    """(b): most nodes' groups broken: group tiles stay a minority and the windows are kept -- claimed group-marked narrow tiles are
    the segment-window kernel's."""
    what = "%d unknowns per node, group minority" % d
    rows, cols, p, c, v = mesh_case(d, broken={2: 0.2, 4: 0.45}[d])
    assert_segment_windows_first(plan_info(rows, cols, p, c, v, flags=capi.FLAG_NO_BLOCK_TILES), what)
    info = check_y(oracle, what, rows, cols, p, c, v)
    assert 0 < info["group_tiles"] <= info["row_blocks"] / 2 and info["segwin_tiles"] > 0, (what, short(info))


@pytest.mark.parametrize("d", [3, 2])
def test_block_windows_given_up_for_a_tile_majority(oracle, d):
    """(d): far couplings in the first 15 % of the nodes only -- too few blocks for segment windows, so the all-narrow 16-tile
    blocks get block windows; then block / group tiles take most of the tiles and the block windows are dropped."""
    what = "%d unknowns per node, block windows then a tile majority" % d
    rows, cols, p, c, v = mesh_case(d, far_share=0.15)
    info_n = plan_info(rows, cols, p, c, v, flags=capi.FLAG_NO_BLOCK_TILES)
    assert info_n["segwin_tiles"] == 0 and info_n["blockwin_tiles"] > 0 and 0 < info_n["narrow_tiles"] < info_n["row_blocks"], (what, short(info_n))
    info = check_y(oracle, what, rows, cols, p, c, v, other_columns_bits=d in (2, 4))
    assert tiles_of(info, d) > info["row_blocks"] / 2 and info["blockwin_tiles"] == 0, (what, short(info))


STAR7 = [(0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)]


def grid7(shape, levels, seed=5):
    """A 7-point grid, one unknown per cell, values from a dictionary of `levels`: ascending columns."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    idx = np.indices(shape).reshape(3, -1)
    strides = np.array([shape[1] * shape[2], shape[2], 1])
    cols = [np.arange(n)]
    ok = [np.ones(n, dtype=bool)]
    for off in STAR7:
        nb = idx + np.array(off)[:, None]
        ok.append(np.all((nb >= 0) & (nb < np.array(shape)[:, None]), axis=0))
        cols.append(np.where(ok[-1], (nb * strides[:, None]).sum(axis=0), 0))
    cols, ok = np.stack(cols, axis=1), np.stack(ok, axis=1)
    order = np.argsort(cols + np.where(ok, 0, 1 << 40), axis=1, kind="stable")
    cols, ok = np.take_along_axis(cols, order, axis=1), np.take_along_axis(ok, order, axis=1)
    lens = ok.sum(axis=1)
    p = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=p[1:])
    c = cols[ok].astype(np.int32)
    v = rng.choice(rng.uniform(-1.0, 1.0, size=levels), size=len(c))
    return n, n, p.astype(np.int32), c, v


def test_grid_windows_given_up_for_stencil_tiles(oracle):
    """(e): a 7-point grid with lines so short that 16 tiles span fewer than 8192 columns gets block windows; masked stencil tiles
    then make most of the matrix column-free and the windows go.  A dictionary (100 values) asked for before the repack is asked
    for again: both orders of the calls end in the same plan."""
    what = "7-point 33 x 47 x 29"
    rows, cols, p, c, v = grid7((29, 47, 33), 100)
    info_n = plan_info(rows, cols, p, c, v, flags=capi.FLAG_NO_SHIFTED_TILES, index_values="after")
    assert info_n["segwin_tiles"] + info_n["blockwin_tiles"] > 0 and 0 < info_n["narrow_tiles"], (what, short(info_n))
    infos = {}
    for order in ("after", "before"):
        infos[order] = check_y(oracle, what + ", index_values " + order, rows, cols, p, c, v, index_values=order)
        info = infos[order]
        assert info["stencil_mask_tiles"] > 0 and info["segwin_tiles"] == 0 and info["blockwin_tiles"] == 0, (what, order, short(info))
        assert info["shifted_tiles"] + info["stencil_mask_tiles"] > info["row_blocks"] / 2 and info["indexed_values"] == 100, (what, order, short(info))
    for k in ("stencil_mask_tiles", "indexed_values", "row_blocks", "value_row_tiles", "dictionary_launch_tiles", "streamed_bytes"):
        assert infos["before"][k] == infos["after"][k], (k, infos["before"][k], infos["after"][k])
