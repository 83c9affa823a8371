"""`spmv-cache-trace-hip --vectors K` without a GPU: every combination it cannot run is refused while the options are parsed
(argp: exit status 64, one line naming the reason), and with no usable device it fails instead of running anything in its
place."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spmv-cache-trace_amd", "spmv-cache-trace-hip")
GENERAL = os.path.join(ROOT, "tests", "golden", "poisson2D.mtx")
BUS = os.path.join(ROOT, "tests", "golden", "bus1138_like.mtx")


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("SPMV_DEVICE", None)
    if env:
        e.update(env)
    return subprocess.run([CLI] + args + ["--threads", "1", "--profile", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120, env=e)


@pytest.mark.parametrize("args, message", [
    (["--csr", GENERAL, "--vectors", "0"], "vectors: expected an integer from 1 to 16"),
    (["--csr", GENERAL, "--vectors", "17"], "vectors: expected an integer from 1 to 16"),
    (["--csr", GENERAL, "--vectors", "-3"], "vectors: expected an integer from 1 to 16"),
    (["--csr", GENERAL, "--vectors", "four"], "vectors: expected an integer from 1 to 16"),
    (["--spmv-format", "coo", "-m", GENERAL, "--vectors", "4"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-coo", "-m", GENERAL, "--vectors", "4"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-ell", "-m", GENERAL, "--vectors", "4"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-hybrid", "-m", GENERAL, "--vectors", "4"], "needs the CSR kernel on the GPU"),
    (["--coo", GENERAL, "--vectors", "4"], "needs the CSR kernel on the GPU"),
    (["--vectors", "4", "--triad", "1000"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "csr", "-m", GENERAL, "--vectors", "4"], "no CPU multi-vector kernel"),
    (["--csr", GENERAL, "--device", "cpu", "--vectors", "4"], "no CPU multi-vector kernel"),
    (["--csr", GENERAL, "--vectors", "4", "--gpus", "2"], "--gpus must be 1"),
    (["--spmv-format", "hip-csr", "-m", GENERAL, "--vectors", "2", "--gpus", "8"], "runs on one device"),
    (["--csr", BUS, "--vectors", "4", "--symmetric"], "cannot be combined with --symmetric"),
])
def test_refused_while_parsing(args, message):
    r = _run(args)
    assert r.returncode == 64, (r.returncode, r.stderr)
    assert message in r.stderr, r.stderr
    assert r.stdout == ""


def test_accepted_combinations_pass_the_parser():
    for args in (["--csr", GENERAL, "--vectors", "4"], ["--spmv-format", "hip-csr", "-m", GENERAL, "--vectors", "16"],
                 ["--csr", "synthetic:queen:4,4,4", "--vectors", "1", "--gpus", "1"], ["--device", "hip", "--csr", GENERAL, "--vectors", "3"]):
        r = _run(args)
        assert r.returncode != 64, (args, r.stderr)


def test_without_a_device_it_fails_and_does_not_fall_back():
    from spmv_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present: this covers the box without one")
    for args in (["--csr", GENERAL, "--vectors", "4"], ["--spmv-format", "hip-csr", "-m", GENERAL, "--vectors", "4"],
                 ["--csr", "synthetic:queen:4,4,4", "--vectors", "8", "--check"]):
        r = _run(args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert r.stdout == "", r.stdout  # no JSON document: nothing ran
        assert "no CPU" in r.stderr or "no HIP device" in r.stderr, r.stderr
        assert "the CPU (OpenMP) kernel runs" not in r.stderr
    r = _run(["--csr", GENERAL, "--vectors", "4"], env={"SPMV_DEVICE": "cpu"})
    assert r.returncode == 1 and r.stdout == "" and "no CPU multi-vector kernel" in r.stderr


def test_help_names_the_option():
    r = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "--vectors" in r.stdout
