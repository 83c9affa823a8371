"""The order and the text of every argument refusal of the float-tile multiplies (formats 7 to 10) on the MI355X: the twelve
Level-2 entry points spmv_hip_csr_spmv_{f32,c16,c16_f64,c16_f32xy}{,_scaled,_scaled_dots}, the four Level-1 uploads of these
formats, and the uploads of formats 5 and 6 as far as they share a prelude with them.

A ladder is the list of what an entry point refuses, in the order it refuses it.  It is walked one rung at a time: a call breaks
rung k AND the next rung that can be broken beside it without mending rung k (two rungs that need the same argument cannot be:
d_y_out cannot both be d_x and be null, and d_x cannot be d_y and null), and must answer with the code and the full
spmv_hip_last_error text of rung k.  After every refused call the
vectors of the call still hold their sentinel bits and a context of the same family still multiplies the matrix it held to the
bits it gave before.  Nothing is provoked beyond refusals: every call here returns before any launch.

EXPECTED was written by collect() on the library built from the commit BEFORE the multiplies were given one host front
(tile_front.hpp), not read off the code that is tested here; that library passes this file unchanged."""
import numpy as np
import pytest

import compact_cases as cc
from spmv_amd import capi

pytestmark = pytest.mark.gpu

KINDS = ("f32", "c16", "c16_f64", "c16_f32xy")
SHAPES = ("plain", "scaled", "scaled_dots")
UPLOADS = {"f32": "spmv_hip_upload_csr_f32values", "c16": "spmv_hip_upload_csr_compact", "c16_f64": "spmv_hip_upload_csr_compact_f64",
           "c16_f32xy": "spmv_hip_upload_csr_compact_f32xy"}
SENTINEL = -7.25


def _small():
    return 3, 4, np.array([0, 1, 2, 3], dtype=np.int32), np.array([0, 3, 2], dtype=np.int32), np.array([1.0, 2.0, -0.5])


def _matrices():
    """The 3 x 4 matrix of test_compact_capi.py, a plan with rows and no entries, and the smallest compact case with a wide tile
    (nine_windows, 360 entries; the next, dense_row_9000_wide, has 13492; collect() asserts that the plan has one)."""
    return {"3x4": _small(), "no_entries": (3, 4, np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0)),
            "wide": cc.matrix("nine_windows")[:5]}


class Level2:
    """One family on one matrix: the plan, the device arrays, vectors filled with the sentinel, and the good arguments."""

    def __init__(self, kind, matrix):
        import torch
        self.kind, self.lib = kind, capi.load()
        rows, cols, p, c, v = matrix
        self.f32xy = kind == "c16_f32xy"
        vt = torch.float32 if self.f32xy else torch.float64
        self.es = 4 if self.f32xy else 8
        dev = "cuda:0"
        self.plan = capi.F32Plan(rows, cols, p, 0) if kind == "f32" else capi.C16Plan(rows, cols, p, c, 0)
        self.info = self.plan.info()
        self.keep = [torch.from_numpy(p).to(dev), torch.from_numpy(np.append(c, [0] * 8).astype(np.int32)).to(dev),
                     torch.from_numpy(np.append(v, [0.0] * 8)).to(dev).to(torch.float64 if kind == "c16_f64" else torch.float32),
                     torch.ones(cols + 8, dtype=vt, device=dev)]
        self.y_in = torch.full((rows + 8,), SENTINEL, dtype=vt, device=dev)
        self.y_out = torch.full((2 * rows + 8,), SENTINEL, dtype=vt, device=dev)
        self.w = torch.ones(rows + 8, dtype=vt, device=dev)
        self.work_bytes = self.plan.dots_workspace_bytes()
        self.dots = torch.zeros(2, dtype=torch.float64, device=dev)
        self.work = torch.zeros(self.work_bytes // 8, dtype=torch.float64, device=dev)
        self.want_in, self.want_out = self.y_in.clone(), self.y_out.clone()
        self.good = dict(plan=self.plan.h, rp=self.keep[0].data_ptr(), ci=self.keep[1].data_ptr(), val=self.keep[2].data_ptr(),
                         x=self.keep[3].data_ptr(), alpha=1.25, beta=-0.5, y_in=self.y_in.data_ptr(), y_out=self.y_out.data_ptr(),
                         w=self.w.data_ptr(), dots=self.dots.data_ptr(), work=self.work.data_ptr(), work_bytes=self.work_bytes)

    def ladder(self, shape):
        """(name, the arguments it changes) in the order of refusal."""
        es, g = self.es, self.good
        # (x is named among the arguments of "x is y", so that no rung that moves x is broken beside it)
        r = [("plan null", dict(plan=None)), ("x is y", dict(x=g["x"], y_out=g["x"]))]
        if shape != "plain":
            r += [("y_out null", dict(y_out=None))]
            if self.f32xy:
                r += [("y_out off 4 bytes", dict(y_out=g["y_out"] + 2))]
            r += [("y_in null, beta != 0", dict(y_in=None, beta=0.5)), ("y_in overlaps y_out", dict(y_in=g["y_out"] + es))]
        if shape == "scaled_dots":
            r += [("dots null", dict(dots=None)), ("work too small", dict(work_bytes=0)), ("dots off 16 bytes", dict(dots=g["dots"] + 8))]
            if self.f32xy:
                r += [("w off 4 bytes", dict(w=g["w"] + 2))]
            r += [("w overlaps y_out", dict(w=g["y_out"])), ("dots overlaps work", dict(dots=g["dots"], work=g["dots"])),
                  ("dots overlaps row_ptr", dict(dots=g["rp"]))]
        if self.info["tiles"] > 0:  # (a plan without tiles reads no array: nothing further is refused)
            r += [("x null", dict(x=None))]
            if self.kind == "f32" or self.info["wide_tiles"] > 0:
                r += [("columns null", dict(ci=None))]
            r += [("values off 16 bytes", dict(val=g["val"] + 8))]
            if self.f32xy:
                r += [("x off 4 bytes", dict(x=g["x"] + 2))]
        return r

    def call(self, shape, a):
        name = {"f32": "spmv_hip_csr_spmv_f32", "c16": "spmv_hip_csr_spmv_c16", "c16_f64": "spmv_hip_csr_spmv_c16_f64",
                "c16_f32xy": "spmv_hip_csr_spmv_c16_f32xy"}[self.kind] + {"plain": "", "scaled": "_scaled", "scaled_dots": "_scaled_dots"}[shape]
        head = (a["plan"], a["rp"], a["ci"], a["val"], a["x"])
        if shape == "plain":
            args = head + (a["y_out"], None)
        elif shape == "scaled":
            args = head + (a["alpha"], a["beta"], a["y_in"], a["y_out"], None)
        else:
            args = head + (a["alpha"], a["beta"], a["y_in"], a["y_out"], a["w"], a["dots"], a["work"], a["work_bytes"], None)
        rc = getattr(self.lib, name)(*args)
        return rc, self.lib.spmv_hip_last_error().decode()

    def untouched(self, what):
        import torch
        assert torch.equal(self.y_in.view(torch.uint8), self.want_in.view(torch.uint8)), what + ": y_in was written"
        assert torch.equal(self.y_out.view(torch.uint8), self.want_out.view(torch.uint8)), what + ": y was written"

    def close(self):
        self.plan.close()


class Held:
    """A context of one family that holds the 3 x 4 matrix: still() multiplies it again and compares the bits of y."""

    def __init__(self, kind, flags=0):
        self.ctx = capi.Context(0, flags)
        self.f32xy = kind == "c16_f32xy"
        rows, cols, p, c, v = _small()
        if kind == "c16_f64":
            self.ctx.upload_csr_compact_f64(rows, cols, p, c, v)
        else:
            getattr(self.ctx, UPLOADS[kind][len("spmv_hip_"):])(rows, cols, p, c, v, allow_rounding=False)
        self.x, self.y0 = np.array([1.0, -2.0, 0.5, 3.0]), np.array([0.25, 0.5, -1.0])
        if self.f32xy:
            self.x, self.y0 = self.x.astype(np.float32), self.y0.astype(np.float32)
        (self.ctx.set_x_f32 if self.f32xy else self.ctx.set_x)(self.x)
        self.want = self._run()

    def _run(self):
        (self.ctx.set_y_f32 if self.f32xy else self.ctx.set_y)(self.y0)
        self.ctx.run()
        return (self.ctx.get_y_f32 if self.f32xy else self.ctx.get_y)().copy()

    def still(self, what):
        got = self._run()
        assert got.tobytes() == self.want.tobytes(), what + ": the context no longer multiplies its matrix to the same bits"

    def close(self):
        self.ctx.close()


def _walk(ladder, good, call, after, tag):
    """Break rung k and the next rung whose arguments are not rung k's; the answer is rung k's."""
    out = []
    for k, (name, change) in enumerate(ladder):
        args = dict(good)
        beside = next((c for _, c in ladder[k + 1:] if not set(c) & set(change)), {})
        args.update(beside)
        args.update(change)
        rc, text = call(args)
        assert rc != capi.OK, (tag, name)
        after("%s, %s" % (tag, name))
        out.append(("%s, %s" % (tag, name), rc, text))
    return out


def _upload_ladder(kind, held, multi, exact):
    rows, cols, p, c, v = _small()
    bad_rp, high = np.array([1, 1, 2, 3], dtype=np.int32), np.array([0, 4, 2], dtype=np.int32)
    keep = [p, c, v, bad_rp, high, np.array([1e300, 1.0, 1.0]), np.array([0.1, 1.0, 1.0])]
    good = dict(ctx=held.ctx.h, rows=rows, cols=cols, nnz=3, rp=p.ctypes.data, ci=c.ctypes.data, val=v.ctypes.data, allow=0)
    r = [("ctx null", dict(ctx=None)), ("multi-GPU context", dict(ctx=multi.h))]
    if kind in ("symmetric", "transposed"):
        r += [("exact order", dict(ctx=exact.h)), ("nnz < 0", dict(nnz=-1)), ("row_ptr[0] != 0", dict(rp=bad_rp.ctypes.data))]
    else:
        r += [("nnz < 0", dict(nnz=-1)), ("row_ptr[0] != 0", dict(rp=bad_rp.ctypes.data)), ("row_ptr[rows] != nnz", dict(nnz=2)),
              ("column out of range", dict(ci=high.ctypes.data))]
        if kind != "c16_f64":
            r += [("a value overflows float", dict(val=keep[5].ctypes.data)), ("a value is no float", dict(val=keep[6].ctypes.data))]
    return r, good, keep


def _upload_call(lib, kind, a):
    if kind == "symmetric":
        rc = lib.spmv_hip_upload_csr_symmetric(a["ctx"], a["rows"], a["nnz"], a["rp"], a["ci"], a["val"], capi.SYMMETRIC)
    elif kind == "transposed":
        rc = lib.spmv_hip_upload_csr_transposed(a["ctx"], a["rows"], a["cols"], a["nnz"], a["rp"], a["ci"], a["val"])
    elif kind == "c16_f64":
        rc = lib.spmv_hip_upload_csr_compact_f64(a["ctx"], a["rows"], a["cols"], a["nnz"], a["rp"], a["ci"], a["val"])
    else:
        rc = getattr(lib, UPLOADS[kind])(a["ctx"], a["rows"], a["cols"], a["nnz"], a["rp"], a["ci"], a["val"], a["allow"])
    return rc, lib.spmv_hip_last_error().decode()


def collect():
    """Every ladder walked; [(what, code, text)]."""
    lib = capi.load()
    out = []
    matrices = _matrices()
    assert capi.c16_plan_preview(*matrices["wide"][:4], table=False)[0]["wide_tiles"] > 0
    multi, exact = capi.Context(num_gpus=1), capi.Context(0, capi.FLAG_EXACT_ORDER)
    held = {kind: Held(kind) for kind in KINDS}
    for kind in KINDS:
        for mname, m in matrices.items():
            dev = Level2(kind, m)
            if mname == "wide" and kind != "f32":
                assert dev.info["wide_tiles"] > 0

            def after(what, dev=dev, kind=kind):
                dev.untouched(what)
                held[kind].still(what)

            for shape in SHAPES:
                out += _walk(dev.ladder(shape), dev.good, lambda a, dev=dev, shape=shape: dev.call(shape, a), after,
                             "%s%s on %s" % (kind, "" if shape == "plain" else "_" + shape, mname))
            dev.close()
    for kind in KINDS + ("symmetric", "transposed"):
        h = held[kind if kind in KINDS else "f32"]
        ladder, good, keep = _upload_ladder(kind, h, multi, exact)
        out += _walk(ladder, good, lambda a, kind=kind: _upload_call(lib, kind, a), h.still, "upload %s" % kind)
    for h in held.values():
        h.close()
    multi.close()
    exact.close()
    return out


EXPECTED = [
    ('f32 on 3x4, plan null', -1, 'plan is null'),
    ('f32 on 3x4, x is y', -1, 'd_x and d_y must be different arrays'),
    ('f32 on 3x4, x null', -1, 'null device pointer'),
    ('f32 on 3x4, columns null', -1, 'null device pointer'),
    ('f32 on 3x4, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('f32_scaled on 3x4, plan null', -1, 'plan is null'),
    ('f32_scaled on 3x4, x is y', -1, 'd_x and d_y must be different arrays'),
    ('f32_scaled on 3x4, y_out null', -1, 'd_y_out is null'),
    ('f32_scaled on 3x4, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('f32_scaled on 3x4, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('f32_scaled on 3x4, x null', -1, 'null device pointer'),
    ('f32_scaled on 3x4, columns null', -1, 'null device pointer'),
    ('f32_scaled on 3x4, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('f32_scaled_dots on 3x4, plan null', -1, 'plan is null'),
    ('f32_scaled_dots on 3x4, x is y', -1, 'd_x and d_y must be different arrays'),
    ('f32_scaled_dots on 3x4, y_out null', -1, 'd_y_out is null'),
    ('f32_scaled_dots on 3x4, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('f32_scaled_dots on 3x4, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('f32_scaled_dots on 3x4, dots null', -1, 'd_dots or d_work is null'),
    ('f32_scaled_dots on 3x4, work too small', -1, 'work_bytes is 0 and the plan needs 32 (spmv_hip_*_dots_workspace)'),
    ('f32_scaled_dots on 3x4, dots off 16 bytes', -7, 'd_dots and d_work must be 16-byte aligned'),
    ('f32_scaled_dots on 3x4, w overlaps y_out', -1, 'd_w overlaps d_y_out'),
    ('f32_scaled_dots on 3x4, dots overlaps work', -1, 'd_dots and d_work overlap'),
    ('f32_scaled_dots on 3x4, dots overlaps row_ptr', -1, 'd_dots or d_work overlaps an array of the call'),
    ('f32_scaled_dots on 3x4, x null', -1, 'null device pointer'),
    ('f32_scaled_dots on 3x4, columns null', -1, 'null device pointer'),
    ('f32_scaled_dots on 3x4, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('f32 on no_entries, plan null', -1, 'plan is null'),
    ('f32 on no_entries, x is y', -1, 'd_x and d_y must be different arrays'),
    ('f32_scaled on no_entries, plan null', -1, 'plan is null'),
    ('f32_scaled on no_entries, x is y', -1, 'd_x and d_y must be different arrays'),
    ('f32_scaled on no_entries, y_out null', -1, 'd_y_out is null'),
    ('f32_scaled on no_entries, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('f32_scaled on no_entries, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('f32_scaled_dots on no_entries, plan null', -1, 'plan is null'),
    ('f32_scaled_dots on no_entries, x is y', -1, 'd_x and d_y must be different arrays'),
    ('f32_scaled_dots on no_entries, y_out null', -1, 'd_y_out is null'),
    ('f32_scaled_dots on no_entries, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('f32_scaled_dots on no_entries, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('f32_scaled_dots on no_entries, dots null', -1, 'd_dots or d_work is null'),
    ('f32_scaled_dots on no_entries, work too small', -1, 'work_bytes is 0 and the plan needs 32 (spmv_hip_*_dots_workspace)'),
    ('f32_scaled_dots on no_entries, dots off 16 bytes', -7, 'd_dots and d_work must be 16-byte aligned'),
    ('f32_scaled_dots on no_entries, w overlaps y_out', -1, 'd_w overlaps d_y_out'),
    ('f32_scaled_dots on no_entries, dots overlaps work', -1, 'd_dots and d_work overlap'),
    ('f32_scaled_dots on no_entries, dots overlaps row_ptr', -1, 'd_dots or d_work overlaps an array of the call'),
    ('f32 on wide, plan null', -1, 'plan is null'),
    ('f32 on wide, x is y', -1, 'd_x and d_y must be different arrays'),
    ('f32 on wide, x null', -1, 'null device pointer'),
    ('f32 on wide, columns null', -1, 'null device pointer'),
    ('f32 on wide, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('f32_scaled on wide, plan null', -1, 'plan is null'),
    ('f32_scaled on wide, x is y', -1, 'd_x and d_y must be different arrays'),
    ('f32_scaled on wide, y_out null', -1, 'd_y_out is null'),
    ('f32_scaled on wide, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('f32_scaled on wide, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('f32_scaled on wide, x null', -1, 'null device pointer'),
    ('f32_scaled on wide, columns null', -1, 'null device pointer'),
    ('f32_scaled on wide, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('f32_scaled_dots on wide, plan null', -1, 'plan is null'),
    ('f32_scaled_dots on wide, x is y', -1, 'd_x and d_y must be different arrays'),
    ('f32_scaled_dots on wide, y_out null', -1, 'd_y_out is null'),
    ('f32_scaled_dots on wide, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('f32_scaled_dots on wide, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('f32_scaled_dots on wide, dots null', -1, 'd_dots or d_work is null'),
    ('f32_scaled_dots on wide, work too small', -1, 'work_bytes is 0 and the plan needs 32 (spmv_hip_*_dots_workspace)'),
    ('f32_scaled_dots on wide, dots off 16 bytes', -7, 'd_dots and d_work must be 16-byte aligned'),
    ('f32_scaled_dots on wide, w overlaps y_out', -1, 'd_w overlaps d_y_out'),
    ('f32_scaled_dots on wide, dots overlaps work', -1, 'd_dots and d_work overlap'),
    ('f32_scaled_dots on wide, dots overlaps row_ptr', -1, 'd_dots or d_work overlaps an array of the call'),
    ('f32_scaled_dots on wide, x null', -1, 'null device pointer'),
    ('f32_scaled_dots on wide, columns null', -1, 'null device pointer'),
    ('f32_scaled_dots on wide, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16 on 3x4, plan null', -1, 'plan is null'),
    ('c16 on 3x4, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16 on 3x4, x null', -1, 'null device pointer'),
    ('c16 on 3x4, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_scaled on 3x4, plan null', -1, 'plan is null'),
    ('c16_scaled on 3x4, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_scaled on 3x4, y_out null', -1, 'd_y_out is null'),
    ('c16_scaled on 3x4, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_scaled on 3x4, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_scaled on 3x4, x null', -1, 'null device pointer'),
    ('c16_scaled on 3x4, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_scaled_dots on 3x4, plan null', -1, 'plan is null'),
    ('c16_scaled_dots on 3x4, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_scaled_dots on 3x4, y_out null', -1, 'd_y_out is null'),
    ('c16_scaled_dots on 3x4, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_scaled_dots on 3x4, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_scaled_dots on 3x4, dots null', -1, 'd_dots or d_work is null'),
    ('c16_scaled_dots on 3x4, work too small', -1, 'work_bytes is 0 and the plan needs 32 (spmv_hip_*_dots_workspace)'),
    ('c16_scaled_dots on 3x4, dots off 16 bytes', -7, 'd_dots and d_work must be 16-byte aligned'),
    ('c16_scaled_dots on 3x4, w overlaps y_out', -1, 'd_w overlaps d_y_out'),
    ('c16_scaled_dots on 3x4, dots overlaps work', -1, 'd_dots and d_work overlap'),
    ('c16_scaled_dots on 3x4, dots overlaps row_ptr', -1, 'd_dots or d_work overlaps an array of the call'),
    ('c16_scaled_dots on 3x4, x null', -1, 'null device pointer'),
    ('c16_scaled_dots on 3x4, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16 on no_entries, plan null', -1, 'plan is null'),
    ('c16 on no_entries, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_scaled on no_entries, plan null', -1, 'plan is null'),
    ('c16_scaled on no_entries, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_scaled on no_entries, y_out null', -1, 'd_y_out is null'),
    ('c16_scaled on no_entries, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_scaled on no_entries, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_scaled_dots on no_entries, plan null', -1, 'plan is null'),
    ('c16_scaled_dots on no_entries, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_scaled_dots on no_entries, y_out null', -1, 'd_y_out is null'),
    ('c16_scaled_dots on no_entries, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_scaled_dots on no_entries, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_scaled_dots on no_entries, dots null', -1, 'd_dots or d_work is null'),
    ('c16_scaled_dots on no_entries, work too small', -1, 'work_bytes is 0 and the plan needs 32 (spmv_hip_*_dots_workspace)'),
    ('c16_scaled_dots on no_entries, dots off 16 bytes', -7, 'd_dots and d_work must be 16-byte aligned'),
    ('c16_scaled_dots on no_entries, w overlaps y_out', -1, 'd_w overlaps d_y_out'),
    ('c16_scaled_dots on no_entries, dots overlaps work', -1, 'd_dots and d_work overlap'),
    ('c16_scaled_dots on no_entries, dots overlaps row_ptr', -1, 'd_dots or d_work overlaps an array of the call'),
    ('c16 on wide, plan null', -1, 'plan is null'),
    ('c16 on wide, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16 on wide, x null', -1, 'null device pointer'),
    ('c16 on wide, columns null', -1, 'd_column_index is null and the plan has wide tiles, which read the 32-bit columns'),
    ('c16 on wide, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_scaled on wide, plan null', -1, 'plan is null'),
    ('c16_scaled on wide, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_scaled on wide, y_out null', -1, 'd_y_out is null'),
    ('c16_scaled on wide, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_scaled on wide, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_scaled on wide, x null', -1, 'null device pointer'),
    ('c16_scaled on wide, columns null', -1, 'd_column_index is null and the plan has wide tiles, which read the 32-bit columns'),
    ('c16_scaled on wide, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_scaled_dots on wide, plan null', -1, 'plan is null'),
    ('c16_scaled_dots on wide, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_scaled_dots on wide, y_out null', -1, 'd_y_out is null'),
    ('c16_scaled_dots on wide, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_scaled_dots on wide, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_scaled_dots on wide, dots null', -1, 'd_dots or d_work is null'),
    ('c16_scaled_dots on wide, work too small', -1, 'work_bytes is 0 and the plan needs 32 (spmv_hip_*_dots_workspace)'),
    ('c16_scaled_dots on wide, dots off 16 bytes', -7, 'd_dots and d_work must be 16-byte aligned'),
    ('c16_scaled_dots on wide, w overlaps y_out', -1, 'd_w overlaps d_y_out'),
    ('c16_scaled_dots on wide, dots overlaps work', -1, 'd_dots and d_work overlap'),
    ('c16_scaled_dots on wide, dots overlaps row_ptr', -1, 'd_dots or d_work overlaps an array of the call'),
    ('c16_scaled_dots on wide, x null', -1, 'null device pointer'),
    ('c16_scaled_dots on wide, columns null', -1, 'd_column_index is null and the plan has wide tiles, which read the 32-bit columns'),
    ('c16_scaled_dots on wide, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f64 on 3x4, plan null', -1, 'plan is null'),
    ('c16_f64 on 3x4, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f64 on 3x4, x null', -1, 'null device pointer'),
    ('c16_f64 on 3x4, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f64_scaled on 3x4, plan null', -1, 'plan is null'),
    ('c16_f64_scaled on 3x4, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f64_scaled on 3x4, y_out null', -1, 'd_y_out is null'),
    ('c16_f64_scaled on 3x4, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_f64_scaled on 3x4, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_f64_scaled on 3x4, x null', -1, 'null device pointer'),
    ('c16_f64_scaled on 3x4, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f64_scaled_dots on 3x4, plan null', -1, 'plan is null'),
    ('c16_f64_scaled_dots on 3x4, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f64_scaled_dots on 3x4, y_out null', -1, 'd_y_out is null'),
    ('c16_f64_scaled_dots on 3x4, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_f64_scaled_dots on 3x4, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_f64_scaled_dots on 3x4, dots null', -1, 'd_dots or d_work is null'),
    ('c16_f64_scaled_dots on 3x4, work too small', -1, 'work_bytes is 0 and the plan needs 32 (spmv_hip_*_dots_workspace)'),
    ('c16_f64_scaled_dots on 3x4, dots off 16 bytes', -7, 'd_dots and d_work must be 16-byte aligned'),
    ('c16_f64_scaled_dots on 3x4, w overlaps y_out', -1, 'd_w overlaps d_y_out'),
    ('c16_f64_scaled_dots on 3x4, dots overlaps work', -1, 'd_dots and d_work overlap'),
    ('c16_f64_scaled_dots on 3x4, dots overlaps row_ptr', -1, 'd_dots or d_work overlaps an array of the call'),
    ('c16_f64_scaled_dots on 3x4, x null', -1, 'null device pointer'),
    ('c16_f64_scaled_dots on 3x4, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f64 on no_entries, plan null', -1, 'plan is null'),
    ('c16_f64 on no_entries, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f64_scaled on no_entries, plan null', -1, 'plan is null'),
    ('c16_f64_scaled on no_entries, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f64_scaled on no_entries, y_out null', -1, 'd_y_out is null'),
    ('c16_f64_scaled on no_entries, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_f64_scaled on no_entries, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_f64_scaled_dots on no_entries, plan null', -1, 'plan is null'),
    ('c16_f64_scaled_dots on no_entries, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f64_scaled_dots on no_entries, y_out null', -1, 'd_y_out is null'),
    ('c16_f64_scaled_dots on no_entries, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_f64_scaled_dots on no_entries, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_f64_scaled_dots on no_entries, dots null', -1, 'd_dots or d_work is null'),
    ('c16_f64_scaled_dots on no_entries, work too small', -1, 'work_bytes is 0 and the plan needs 32 (spmv_hip_*_dots_workspace)'),
    ('c16_f64_scaled_dots on no_entries, dots off 16 bytes', -7, 'd_dots and d_work must be 16-byte aligned'),
    ('c16_f64_scaled_dots on no_entries, w overlaps y_out', -1, 'd_w overlaps d_y_out'),
    ('c16_f64_scaled_dots on no_entries, dots overlaps work', -1, 'd_dots and d_work overlap'),
    ('c16_f64_scaled_dots on no_entries, dots overlaps row_ptr', -1, 'd_dots or d_work overlaps an array of the call'),
    ('c16_f64 on wide, plan null', -1, 'plan is null'),
    ('c16_f64 on wide, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f64 on wide, x null', -1, 'null device pointer'),
    ('c16_f64 on wide, columns null', -1, 'd_column_index is null and the plan has wide tiles, which read the 32-bit columns'),
    ('c16_f64 on wide, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f64_scaled on wide, plan null', -1, 'plan is null'),
    ('c16_f64_scaled on wide, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f64_scaled on wide, y_out null', -1, 'd_y_out is null'),
    ('c16_f64_scaled on wide, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_f64_scaled on wide, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_f64_scaled on wide, x null', -1, 'null device pointer'),
    ('c16_f64_scaled on wide, columns null', -1, 'd_column_index is null and the plan has wide tiles, which read the 32-bit columns'),
    ('c16_f64_scaled on wide, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f64_scaled_dots on wide, plan null', -1, 'plan is null'),
    ('c16_f64_scaled_dots on wide, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f64_scaled_dots on wide, y_out null', -1, 'd_y_out is null'),
    ('c16_f64_scaled_dots on wide, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_f64_scaled_dots on wide, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_f64_scaled_dots on wide, dots null', -1, 'd_dots or d_work is null'),
    ('c16_f64_scaled_dots on wide, work too small', -1, 'work_bytes is 0 and the plan needs 32 (spmv_hip_*_dots_workspace)'),
    ('c16_f64_scaled_dots on wide, dots off 16 bytes', -7, 'd_dots and d_work must be 16-byte aligned'),
    ('c16_f64_scaled_dots on wide, w overlaps y_out', -1, 'd_w overlaps d_y_out'),
    ('c16_f64_scaled_dots on wide, dots overlaps work', -1, 'd_dots and d_work overlap'),
    ('c16_f64_scaled_dots on wide, dots overlaps row_ptr', -1, 'd_dots or d_work overlaps an array of the call'),
    ('c16_f64_scaled_dots on wide, x null', -1, 'null device pointer'),
    ('c16_f64_scaled_dots on wide, columns null', -1, 'd_column_index is null and the plan has wide tiles, which read the 32-bit columns'),
    ('c16_f64_scaled_dots on wide, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f32xy on 3x4, plan null', -1, 'plan is null'),
    ('c16_f32xy on 3x4, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f32xy on 3x4, x null', -1, 'null device pointer'),
    ('c16_f32xy on 3x4, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f32xy on 3x4, x off 4 bytes', -7, 'd_x and d_y must be 4-byte aligned'),
    ('c16_f32xy_scaled on 3x4, plan null', -1, 'plan is null'),
    ('c16_f32xy_scaled on 3x4, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f32xy_scaled on 3x4, y_out null', -1, 'd_y_out is null'),
    ('c16_f32xy_scaled on 3x4, y_out off 4 bytes', -7, 'd_y_in and d_y_out must be 4-byte aligned'),
    ('c16_f32xy_scaled on 3x4, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_f32xy_scaled on 3x4, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_f32xy_scaled on 3x4, x null', -1, 'null device pointer'),
    ('c16_f32xy_scaled on 3x4, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f32xy_scaled on 3x4, x off 4 bytes', -7, 'd_x and d_y must be 4-byte aligned'),
    ('c16_f32xy_scaled_dots on 3x4, plan null', -1, 'plan is null'),
    ('c16_f32xy_scaled_dots on 3x4, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f32xy_scaled_dots on 3x4, y_out null', -1, 'd_y_out is null'),
    ('c16_f32xy_scaled_dots on 3x4, y_out off 4 bytes', -7, 'd_y_in and d_y_out must be 4-byte aligned'),
    ('c16_f32xy_scaled_dots on 3x4, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_f32xy_scaled_dots on 3x4, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_f32xy_scaled_dots on 3x4, dots null', -1, 'd_dots or d_work is null'),
    ('c16_f32xy_scaled_dots on 3x4, work too small', -1, 'work_bytes is 0 and the plan needs 32 (spmv_hip_*_dots_workspace)'),
    ('c16_f32xy_scaled_dots on 3x4, dots off 16 bytes', -7, 'd_dots and d_work must be 16-byte aligned'),
    ('c16_f32xy_scaled_dots on 3x4, w off 4 bytes', -7, 'd_w must be 4-byte aligned'),
    ('c16_f32xy_scaled_dots on 3x4, w overlaps y_out', -1, 'd_w overlaps d_y_out'),
    ('c16_f32xy_scaled_dots on 3x4, dots overlaps work', -1, 'd_dots and d_work overlap'),
    ('c16_f32xy_scaled_dots on 3x4, dots overlaps row_ptr', -1, 'd_dots or d_work overlaps an array of the call'),
    ('c16_f32xy_scaled_dots on 3x4, x null', -1, 'null device pointer'),
    ('c16_f32xy_scaled_dots on 3x4, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f32xy_scaled_dots on 3x4, x off 4 bytes', -7, 'd_x and d_y must be 4-byte aligned'),
    ('c16_f32xy on no_entries, plan null', -1, 'plan is null'),
    ('c16_f32xy on no_entries, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f32xy_scaled on no_entries, plan null', -1, 'plan is null'),
    ('c16_f32xy_scaled on no_entries, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f32xy_scaled on no_entries, y_out null', -1, 'd_y_out is null'),
    ('c16_f32xy_scaled on no_entries, y_out off 4 bytes', -7, 'd_y_in and d_y_out must be 4-byte aligned'),
    ('c16_f32xy_scaled on no_entries, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_f32xy_scaled on no_entries, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_f32xy_scaled_dots on no_entries, plan null', -1, 'plan is null'),
    ('c16_f32xy_scaled_dots on no_entries, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f32xy_scaled_dots on no_entries, y_out null', -1, 'd_y_out is null'),
    ('c16_f32xy_scaled_dots on no_entries, y_out off 4 bytes', -7, 'd_y_in and d_y_out must be 4-byte aligned'),
    ('c16_f32xy_scaled_dots on no_entries, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_f32xy_scaled_dots on no_entries, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_f32xy_scaled_dots on no_entries, dots null', -1, 'd_dots or d_work is null'),
    ('c16_f32xy_scaled_dots on no_entries, work too small', -1, 'work_bytes is 0 and the plan needs 32 (spmv_hip_*_dots_workspace)'),
    ('c16_f32xy_scaled_dots on no_entries, dots off 16 bytes', -7, 'd_dots and d_work must be 16-byte aligned'),
    ('c16_f32xy_scaled_dots on no_entries, w off 4 bytes', -7, 'd_w must be 4-byte aligned'),
    ('c16_f32xy_scaled_dots on no_entries, w overlaps y_out', -1, 'd_w overlaps d_y_out'),
    ('c16_f32xy_scaled_dots on no_entries, dots overlaps work', -1, 'd_dots and d_work overlap'),
    ('c16_f32xy_scaled_dots on no_entries, dots overlaps row_ptr', -1, 'd_dots or d_work overlaps an array of the call'),
    ('c16_f32xy on wide, plan null', -1, 'plan is null'),
    ('c16_f32xy on wide, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f32xy on wide, x null', -1, 'null device pointer'),
    ('c16_f32xy on wide, columns null', -1, 'd_column_index is null and the plan has wide tiles, which read the 32-bit columns'),
    ('c16_f32xy on wide, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f32xy on wide, x off 4 bytes', -7, 'd_x and d_y must be 4-byte aligned'),
    ('c16_f32xy_scaled on wide, plan null', -1, 'plan is null'),
    ('c16_f32xy_scaled on wide, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f32xy_scaled on wide, y_out null', -1, 'd_y_out is null'),
    ('c16_f32xy_scaled on wide, y_out off 4 bytes', -7, 'd_y_in and d_y_out must be 4-byte aligned'),
    ('c16_f32xy_scaled on wide, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_f32xy_scaled on wide, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_f32xy_scaled on wide, x null', -1, 'null device pointer'),
    ('c16_f32xy_scaled on wide, columns null', -1, 'd_column_index is null and the plan has wide tiles, which read the 32-bit columns'),
    ('c16_f32xy_scaled on wide, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f32xy_scaled on wide, x off 4 bytes', -7, 'd_x and d_y must be 4-byte aligned'),
    ('c16_f32xy_scaled_dots on wide, plan null', -1, 'plan is null'),
    ('c16_f32xy_scaled_dots on wide, x is y', -1, 'd_x and d_y must be different arrays'),
    ('c16_f32xy_scaled_dots on wide, y_out null', -1, 'd_y_out is null'),
    ('c16_f32xy_scaled_dots on wide, y_out off 4 bytes', -7, 'd_y_in and d_y_out must be 4-byte aligned'),
    ('c16_f32xy_scaled_dots on wide, y_in null, beta != 0', -1, 'd_y_in is null and beta is not 0'),
    ('c16_f32xy_scaled_dots on wide, y_in overlaps y_out', -1, 'd_y_in and d_y_out overlap without being the same array'),
    ('c16_f32xy_scaled_dots on wide, dots null', -1, 'd_dots or d_work is null'),
    ('c16_f32xy_scaled_dots on wide, work too small', -1, 'work_bytes is 0 and the plan needs 32 (spmv_hip_*_dots_workspace)'),
    ('c16_f32xy_scaled_dots on wide, dots off 16 bytes', -7, 'd_dots and d_work must be 16-byte aligned'),
    ('c16_f32xy_scaled_dots on wide, w off 4 bytes', -7, 'd_w must be 4-byte aligned'),
    ('c16_f32xy_scaled_dots on wide, w overlaps y_out', -1, 'd_w overlaps d_y_out'),
    ('c16_f32xy_scaled_dots on wide, dots overlaps work', -1, 'd_dots and d_work overlap'),
    ('c16_f32xy_scaled_dots on wide, dots overlaps row_ptr', -1, 'd_dots or d_work overlaps an array of the call'),
    ('c16_f32xy_scaled_dots on wide, x null', -1, 'null device pointer'),
    ('c16_f32xy_scaled_dots on wide, columns null', -1, 'd_column_index is null and the plan has wide tiles, which read the 32-bit columns'),
    ('c16_f32xy_scaled_dots on wide, values off 16 bytes', -7, 'column / value arrays must be 16-byte aligned'),
    ('c16_f32xy_scaled_dots on wide, x off 4 bytes', -7, 'd_x and d_y must be 4-byte aligned'),
    ('upload f32, ctx null', -1, 'ctx is null'),
    ('upload f32, multi-GPU context', -5, 'the fp32-value multiply runs on one device (a context of spmv_hip_create)'),
    ('upload f32, nnz < 0', -1, 'bad CSR arguments'),
    ('upload f32, row_ptr[0] != 0', -1, 'row_ptr[0] must be 0'),
    ('upload f32, row_ptr[rows] != nnz', -1, 'row_ptr[rows] must equal nnz'),
    ('upload f32, column out of range', -1, 'column index out of range [0, cols)'),
    ('upload f32, a value overflows float', -6, '1 finite value(s) are infinite as floats (the first is entry 0)'),
    ('upload f32, a value is no float', -1, '1 value(s) are not floats (the first is entry 0, relative change at most 1.49e-08) and allow_rounding is 0'),
    ('upload c16, ctx null', -1, 'ctx is null'),
    ('upload c16, multi-GPU context', -5, 'the compact multiply runs on one device (a context of spmv_hip_create)'),
    ('upload c16, nnz < 0', -1, 'bad CSR arguments'),
    ('upload c16, row_ptr[0] != 0', -1, 'row_ptr[0] must be 0'),
    ('upload c16, row_ptr[rows] != nnz', -1, 'row_ptr[rows] must equal nnz'),
    ('upload c16, column out of range', -1, 'column index out of range [0, cols)'),
    ('upload c16, a value overflows float', -6, '1 finite value(s) are infinite as floats (the first is entry 0)'),
    ('upload c16, a value is no float', -1, '1 value(s) are not floats (the first is entry 0, relative change at most 1.49e-08) and allow_rounding is 0'),
    ('upload c16_f64, ctx null', -1, 'ctx is null'),
    ('upload c16_f64, multi-GPU context', -5, 'the compact multiply runs on one device (a context of spmv_hip_create)'),
    ('upload c16_f64, nnz < 0', -1, 'bad CSR arguments'),
    ('upload c16_f64, row_ptr[0] != 0', -1, 'row_ptr[0] must be 0'),
    ('upload c16_f64, row_ptr[rows] != nnz', -1, 'row_ptr[rows] must equal nnz'),
    ('upload c16_f64, column out of range', -1, 'column index out of range [0, cols)'),
    ('upload c16_f32xy, ctx null', -1, 'ctx is null'),
    ('upload c16_f32xy, multi-GPU context', -5, 'the compact multiply runs on one device (a context of spmv_hip_create)'),
    ('upload c16_f32xy, nnz < 0', -1, 'bad CSR arguments'),
    ('upload c16_f32xy, row_ptr[0] != 0', -1, 'row_ptr[0] must be 0'),
    ('upload c16_f32xy, row_ptr[rows] != nnz', -1, 'row_ptr[rows] must equal nnz'),
    ('upload c16_f32xy, column out of range', -1, 'column index out of range [0, cols)'),
    ('upload c16_f32xy, a value overflows float', -6, '1 finite value(s) are infinite as floats (the first is entry 0)'),
    ('upload c16_f32xy, a value is no float', -1, '1 value(s) are not floats (the first is entry 0, relative change at most 1.49e-08) and allow_rounding is 0'),
    ('upload symmetric, ctx null', -1, 'ctx is null'),
    ('upload symmetric, multi-GPU context', -5, 'a symmetric multiply runs on one device (spmv_hip_create_multi partitions rows)'),
    ('upload symmetric, exact order', -1, 'SPMV_HIP_FLAG_EXACT_ORDER cannot be kept: a symmetric multiply adds partial sums with atomics'),
    ('upload symmetric, nnz < 0', -1, 'bad CSR arguments'),
    ('upload symmetric, row_ptr[0] != 0', -1, 'row_ptr[0] must be 0'),
    ('upload transposed, ctx null', -1, 'ctx is null'),
    ('upload transposed, multi-GPU context', -5, 'a transposed multiply runs on one device (a row partition would need a reduction of y across devices)'),
    ('upload transposed, exact order', -1, 'SPMV_HIP_FLAG_EXACT_ORDER cannot be kept: a transposed multiply adds its products with atomics'),
    ('upload transposed, nnz < 0', -1, 'bad CSR arguments'),
    ('upload transposed, row_ptr[0] != 0', -1, 'row_ptr[0] must be 0'),
]


def test_every_refusal_in_order_with_its_text():
    got = collect()
    for g in got:
        print(g)
    assert [g[0] for g in got] == [e[0] for e in EXPECTED]
    for g, e in zip(got, EXPECTED):
        assert g == e
