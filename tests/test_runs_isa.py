"""The compiled stencil row-chunk kernel (csr_runs.hpp), read from its gfx950 assembly: once the descriptor is back a chunk issues
every load -- 5 value LDS-DMA, y_in, five x pairs, and the last entry (full chunks) or the row masks (masked chunks) -- with no
vmcnt wait among them, and waits once per path; a workgroup takes 20 KiB of LDS, so 8 waves per SIMD fit.  Needs hipcc, not a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv-cache-trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = """#include "csr_runs.hpp"
template __global__ void spmv::csr_runs_kernel<false, true>(int, int, int, const int4 *, const uint8_t *, spmv::RunPattern,
                                                            const double *, const double *, const double *, double *);
"""
VECTOR_LOAD = re.compile(r"^\s*(global|buffer|flat)_load")


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("runs_isa")
    src, asm = d / "runs.hip", d / "runs.s"
    src.write_text(SRC)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(asm)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    text = asm.read_text()
    start = re.search(r"^_ZN4spmv15csr_runs_kernelILb0ELb1E\S*:", text, re.M)
    assert start, "kernel not in the assembly"
    body = text[start.end():text.index("s_endpgm", start.end())]
    return body.splitlines(), r.stdout


def test_one_wait_per_chunk(compiled):
    lines, _ = compiled
    # the loads in program order, cut at every wait on vector memory
    groups, cur = [], []
    for ln in lines:
        s = ln.split(";")[0].strip()
        if s.startswith("s_waitcnt") and "vmcnt" in s:
            groups.append(cur)
            cur = []
        elif VECTOR_LOAD.match(s):
            cur.append(s.split()[0])
    assert not any(VECTOR_LOAD.match(s) for s in cur), "a vector load after the last vmcnt wait: %s" % cur
    # the masked path's block sits between the DMA and the full path's block (either order is fine): two waits in all, the
    # first after the 5 DMA and one issue block, the second after the other issue block
    assert len(groups) == 2, groups
    dma = [g.count("global_load_lds_dwordx4") for g in groups]
    assert dma == [5, 0], groups
    for g in groups:
        rest = [op for op in g if op != "global_load_lds_dwordx4"]
        assert rest[:6] == ["global_load_dwordx4"] * 6 and len(rest) == 7, g
        assert rest[6] in ("global_load_dwordx2", "global_load_ushort"), g
    assert sorted(g[-1] for g in groups) == ["global_load_dwordx2", "global_load_ushort"]
    # every wait on vector memory waits for all of them: the only ones are the two above
    assert sum(1 for ln in lines if "vmcnt(" in ln.split(";")[0]) == 2


def test_lds_and_occupancy(compiled):
    _, remarks = compiled

    def remark(name):
        m = re.search(r"csr_runs_kernelILb0ELb1E.*?" + re.escape(name) + r":\s*(\d+)", remarks, re.S)
        assert m, name
        return int(m.group(1))

    assert remark("LDS Size [bytes/block]") == 4 * 640 * 8  # 4 waves x 640 doubles
    assert remark("Occupancy [waves/SIMD]") == 8
    assert remark("VGPRs") <= 64
    assert remark("ScratchSize [bytes/lane]") == 0
