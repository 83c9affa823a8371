"""The C ABI of the compact plan from device arrays (include/spmv_hip_compact_device.h) without a GPU: the two functions are
declared in that header and nowhere else, exported and bound, the header is C99 on its own, and every refusal that precedes the
first HIP call is given with made-up addresses -- nothing is dereferenced, no device is needed -- and leaves a sentinel in *plan
untouched."""
import ctypes as C
import os
import re
import subprocess

from spmv_amd import capi

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "spmv_hip_compact_device.h")
NEW = ["spmv_hip_c16_plan_csr_device", "spmv_hip_c16_plan_table"]
INV, ALI = capi.ERR_INVALID, capi.ERR_ALIGN
SENTINEL = 0x5EED5EED0
P, J = 0x10000000, 0x20000000  # made-up device addresses, 16-byte aligned


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text))


def test_symbols_exported_declared_here_alone_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    assert sorted(_declared(HEADER)) == sorted(NEW)
    for s in NEW:
        assert hasattr(lib, s) and s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    for name in sorted(os.listdir(INCLUDE)):
        if name.endswith(".h") and name != os.path.basename(HEADER):
            assert not (_declared(os.path.join(INCLUDE, name)) & set(NEW)), name
    assert callable(capi.C16Plan.from_device) and callable(capi.C16Plan.table)
    assert len(capi.SIGNATURES["spmv_hip_c16_plan_csr_device"][1]) == 7 and len(capi.SIGNATURES["spmv_hip_c16_plan_table"][1]) == 6


def test_header_is_c99_on_its_own_and_neither_the_version_nor_the_info_count_moved():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_compact_device.h"\nint main(void) { return SPMV_HIP_VERSION + SPMV_HIP_C16_INFO + SPMV_HIP_C16_TILE_INTS; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert '#include "spmv_hip_compact.h"' in text and not re.findall(r"#define SPMV_HIP_(VERSION|C16_INFO)", text)
    assert capi.load().spmv_hip_version() == 130 and len(capi.C16_INFO_KEYS) == 20


def test_every_refusal_before_the_first_hip_call_leaves_the_plan_handle_alone():
    lib = capi.load()
    h = C.c_void_p(SENTINEL)
    plan = C.byref(h)
    for args, code, text in [
            ((None, 3, 4, P, J, 0, None), INV, b"plan is null"),
            ((plan, -1, 4, P, J, 0, None), INV, b"rows < 0"),
            ((plan, -2 ** 31, 4, P, J, 0, None), INV, b"rows < 0"),
            ((plan, 3, -1, P, J, 0, None), INV, b"cols < 0"),
            ((plan, 3, 4, P, J, 0x1, None), INV, b"flag"),
            ((plan, 3, 4, P, J, capi.FLAG_EXACT_ORDER | 0x8, None), INV, b"flag"),
            ((plan, 3, 4, P, J, 0x80000000, None), INV, b"flag"),
            ((plan, 3, 4, None, J, 0, None), INV, b"d_row_ptr is null"),
            ((plan, 0, 0, None, None, 0, None), INV, b"d_row_ptr is null"),
            ((plan, 3, 4, P + 1, J, 0, None), ALI, b"4-byte"),
            ((plan, 3, 4, P + 2, J, capi.FLAG_EXACT_ORDER, None), ALI, b"4-byte"),
            ((plan, 3, 4, P, J + 1, 0, None), ALI, b"4-byte"),
            ((plan, 3, 4, P, J + 2, 0, None), ALI, b"4-byte"),
            ((plan, 3, 4, P, J + 3, 0, None), ALI, b"4-byte")]:
        assert lib.spmv_hip_c16_plan_csr_device(*args) == code, args
        assert text in lib.spmv_hip_last_error(), (args, lib.spmv_hip_last_error())
        assert h.value == SENTINEL, args
    # through the class: the code arrives as an exception and no handle is kept
    for kw, code in [(dict(rows=-1), INV), (dict(cols=-1), INV), (dict(flags=0x4), INV), (dict(d_row_ptr=None), INV), (dict(d_row_ptr=0), INV),
                     (dict(d_row_ptr=P + 2), ALI), (dict(d_col=J + 2), ALI)]:
        a = dict(dict(rows=3, cols=4, d_row_ptr=P, d_col=J, flags=0), **kw)
        try:
            capi.C16Plan.from_device(a["rows"], a["cols"], a["d_row_ptr"], a["d_col"], a["flags"])
        except capi.SpmvHipError as e:
            assert e.code == code, (kw, e)
        else:
            raise AssertionError("not refused: %r" % (kw,))


def test_the_table_of_a_null_plan_is_refused():
    lib = capi.load()
    tab = (C.c_int32 * 13)()
    cod = (C.c_uint16 * 4)()
    assert lib.spmv_hip_c16_plan_table(None, tab, 13, cod, 4, None) == INV
    assert b"plan is null" in lib.spmv_hip_last_error()
    assert lib.spmv_hip_c16_plan_table(None, None, 0, None, 0, None) == INV
