"""`spmv-cache-trace-hip --transpose` without a GPU: every combination it cannot run is refused while the options are parsed
(argp: exit status 64, one line naming the reason), and without a usable device it fails instead of running anything in its
place."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spmv-cache-trace_amd", "spmv-cache-trace-hip")
BUS = os.path.join(ROOT, "tests", "golden", "bus1138_like.mtx")          # `symmetric` header
GENERAL = os.path.join(ROOT, "tests", "golden", "poisson2D.mtx")        # `general` header


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("SPMV_DEVICE", None)
    if env:
        e.update(env)
    return subprocess.run([CLI] + args + ["--threads", "1", "--profile", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120, env=e)


@pytest.mark.parametrize("args, message", [
    (["--csr", BUS, "--transpose", "--symmetric"], "cannot be combined with --symmetric"),
    (["--spmv-format", "hip-csr", "-m", "synthetic:queen:4,4,4:tril", "--symmetric", "--transpose"], "cannot be combined with --symmetric"),
    (["--csr", GENERAL, "--transpose", "--vectors", "4"], "cannot be combined with --vectors"),
    (["--csr", GENERAL, "--transpose", "--gpus", "2"], "--gpus must be 1"),
    (["--spmv-format", "hip-csr", "-m", "synthetic:queen:4,4,4", "--transpose", "--gpus", "4"], "runs on one device"),
    (["--spmv-format", "csr", "-m", GENERAL, "--transpose"], "no CPU transposed kernel"),
    (["--csr", GENERAL, "--device", "cpu", "--transpose"], "no CPU transposed kernel"),
    (["--spmv-format", "coo", "-m", GENERAL, "--transpose"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-coo", "-m", GENERAL, "--transpose"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-ell", "-m", GENERAL, "--transpose"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-hybrid", "-m", GENERAL, "--transpose"], "needs the CSR kernel on the GPU"),
    (["--coo", GENERAL, "--transpose"], "needs the CSR kernel on the GPU"),
    (["--transpose", "--triad", "1000"], "needs the CSR kernel on the GPU"),
])
def test_refused_while_parsing(args, message):
    r = _run(args)
    assert r.returncode == 64, (r.returncode, r.stderr)
    assert message in r.stderr, r.stderr
    assert "--transpose" in r.stderr
    assert r.stdout == ""


def test_accepted_combinations_pass_the_parser():
    """What --transpose is for gets past the option checks (it then needs a device: see below)."""
    for args in (["--csr", GENERAL, "--transpose"], ["--spmv-format", "hip-csr", "-m", GENERAL, "--transpose"],
                 ["--csr", "synthetic:queen:4,4,4", "--transpose", "--gpus", "1"], ["--device", "hip", "--csr", BUS, "--transpose"],
                 ["--csr", BUS, "--transpose", "--expand-symmetric", "--check", "--x", "uniform"]):
        r = _run(args)
        assert r.returncode != 64, (args, r.stderr)


def test_without_a_device_it_fails_and_does_not_fall_back():
    from spmv_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present: this covers the box without one")
    for args in (["--csr", GENERAL, "--transpose"], ["--spmv-format", "hip-csr", "-m", GENERAL, "--transpose"],
                 ["--csr", "synthetic:queen:4,4,4", "--transpose", "--check"]):
        r = _run(args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert r.stdout == "", r.stdout  # no JSON document: nothing ran
        assert "no CPU" in r.stderr or "no HIP device" in r.stderr, r.stderr
        assert "the CPU (OpenMP) kernel runs" not in r.stderr
    # SPMV_DEVICE=cpu cannot make it run on the CPU either
    r = _run(["--csr", GENERAL, "--transpose"], env={"SPMV_DEVICE": "cpu"})
    assert r.returncode == 1 and r.stdout == "" and "no CPU transposed kernel" in r.stderr


def test_help_names_the_option():
    r = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "--transpose" in r.stdout
