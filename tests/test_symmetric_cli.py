"""`spmv-cache-trace-hip --symmetric` without a GPU: every combination it cannot run is refused while the options are parsed
(argp: exit status 64, one line naming the reason), and with a stored triangle but no usable device it fails instead of
running anything in its place."""
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
    (["--csr", BUS, "--symmetric", "--expand-symmetric"], "cannot be combined with --expand-symmetric"),
    (["--csr", GENERAL, "--symmetric"], "needs a file with a `symmetric` or `skew-symmetric` header"),
    (["--spmv-format", "hip-csr", "-m", GENERAL, "--symmetric"], "is general"),
    (["--csr", "synthetic:queen:4,4,4", "--symmetric"], "needs a stored triangle"),
    (["--spmv-format", "csr", "-m", BUS, "--symmetric"], "no CPU symmetric kernel"),
    (["--csr", BUS, "--device", "cpu", "--symmetric"], "no CPU symmetric kernel"),
    (["--spmv-format", "coo", "-m", BUS, "--symmetric"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-coo", "-m", BUS, "--symmetric"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-ell", "-m", BUS, "--symmetric"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-hybrid", "-m", BUS, "--symmetric"], "needs the CSR kernel on the GPU"),
    (["--symmetric", "--triad", "1000"], "needs the CSR kernel on the GPU"),
    (["--csr", BUS, "--symmetric", "--gpus", "2"], "--gpus must be 1"),
    (["--spmv-format", "hip-csr", "-m", "synthetic:queen:4,4,4:tril", "--symmetric", "--gpus", "4"], "runs on one device"),
])
def test_refused_while_parsing(args, message):
    r = _run(args)
    assert r.returncode == 64, (r.returncode, r.stderr)
    assert message in r.stderr, r.stderr
    assert r.stdout == ""


def test_accepted_combinations_pass_the_parser():
    """What --symmetric is for gets past the option checks (it then needs a device: see below)."""
    for args in (["--csr", BUS, "--symmetric"], ["--spmv-format", "hip-csr", "-m", BUS, "--symmetric"],
                 ["--csr", "synthetic:queen:4,4,4:tril", "--symmetric", "--gpus", "1"], ["--device", "hip", "--csr", BUS, "--symmetric"]):
        r = _run(args)
        assert r.returncode != 64, (args, r.stderr)


def test_without_a_device_it_fails_and_does_not_fall_back():
    from spmv_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present: this covers the box without one")
    for args in (["--csr", BUS, "--symmetric"], ["--spmv-format", "hip-csr", "-m", BUS, "--symmetric"],
                 ["--csr", "synthetic:queen:4,4,4:tril", "--symmetric", "--check"]):
        r = _run(args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert r.stdout == "", r.stdout  # no JSON document: nothing ran
        assert "no CPU" in r.stderr or "no HIP device" in r.stderr, r.stderr
        assert "the CPU (OpenMP) kernel runs" not in r.stderr
    # SPMV_DEVICE=cpu cannot make it run on the CPU either
    r = _run(["--csr", BUS, "--symmetric"], env={"SPMV_DEVICE": "cpu"})
    assert r.returncode == 1 and r.stdout == "" and "no CPU symmetric kernel" in r.stderr


def test_help_names_the_option():
    r = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "--symmetric" in r.stdout
