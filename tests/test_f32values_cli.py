"""`spmv-cache-trace-hip --f32-values[=round|exact]` without a GPU: every combination it cannot run is refused while the options
are parsed (argp: exit status 64, one line naming the reason), and without a usable device it fails instead of running anything
in its place."""
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
    (["--csr", BUS, "--f32-values", "--symmetric"], "cannot be combined with --symmetric"),
    (["--spmv-format", "hip-csr", "-m", "synthetic:queen:4,4,4:tril", "--symmetric", "--f32-values=exact"], "cannot be combined with --symmetric"),
    (["--csr", GENERAL, "--f32-values", "--transpose"], "cannot be combined with --transpose"),
    (["--csr", GENERAL, "--f32-values=round", "--vectors", "4"], "cannot be combined with --vectors"),
    (["--csr", GENERAL, "--f32-values", "--gpus", "2"], "--gpus must be 1"),
    (["--spmv-format", "hip-csr", "-m", "synthetic:queen:4,4,4", "--f32-values", "--gpus", "4"], "runs on one device"),
    (["--spmv-format", "csr", "-m", GENERAL, "--f32-values"], "no CPU kernel over float values"),
    (["--csr", GENERAL, "--device", "cpu", "--f32-values"], "no CPU kernel over float values"),
    (["--spmv-format", "coo", "-m", GENERAL, "--f32-values"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-coo", "-m", GENERAL, "--f32-values"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-ell", "-m", GENERAL, "--f32-values"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-hybrid", "-m", GENERAL, "--f32-values"], "needs the CSR kernel on the GPU"),
    (["--coo", GENERAL, "--f32-values"], "needs the CSR kernel on the GPU"),
    (["--ell", GENERAL, "--f32-values"], "needs the CSR kernel on the GPU"),
    (["--f32-values", "--triad", "1000"], "needs the CSR kernel on the GPU"),
])
def test_refused_while_parsing(args, message):
    r = _run(args)
    assert r.returncode == 64, (r.returncode, r.stderr)
    assert message in r.stderr, r.stderr
    assert "--f32-values" in r.stderr
    assert r.stdout == ""


def test_an_unknown_mode_is_refused_while_parsing():
    r = _run(["--csr", GENERAL, "--f32-values=nearest"])
    assert r.returncode == 64 and "expected 'round' (the default) or 'exact'" in r.stderr and r.stdout == ""


def test_accepted_combinations_pass_the_parser():
    """What --f32-values is for gets past the option checks (it then needs a device: see below)."""
    for args in (["--csr", GENERAL, "--f32-values"], ["--spmv-format", "hip-csr", "-m", GENERAL, "--f32-values=round"],
                 ["--csr", "synthetic:queen:4,4,4", "--f32-values=exact", "--gpus", "1"], ["--device", "hip", "--csr", BUS, "--f32-values"],
                 ["--csr", BUS, "--f32-values", "--expand-symmetric", "--check", "--x", "uniform"],
                 ["--csr", GENERAL, "--f32-values", "--exact-order"]):
        r = _run(args)
        assert r.returncode != 64, (args, r.stderr)


def test_without_a_device_it_fails_and_does_not_fall_back():
    from spmv_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present: this covers the box without one")
    for args in (["--csr", GENERAL, "--f32-values"], ["--spmv-format", "hip-csr", "-m", GENERAL, "--f32-values=exact"],
                 ["--csr", "synthetic:queen:4,4,4", "--f32-values", "--check"]):
        r = _run(args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert r.stdout == "", r.stdout  # no JSON document: nothing ran
        assert "no CPU" in r.stderr or "no HIP device" in r.stderr, r.stderr
        assert "the CPU (OpenMP) kernel runs" not in r.stderr
    # SPMV_DEVICE=cpu cannot make it run on the CPU either
    r = _run(["--csr", GENERAL, "--f32-values"], env={"SPMV_DEVICE": "cpu"})
    assert r.returncode == 1 and r.stdout == "" and "no CPU kernel over float values" in r.stderr


def test_help_names_the_option():
    r = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "--f32-values" in r.stdout and "round|exact" in r.stdout
