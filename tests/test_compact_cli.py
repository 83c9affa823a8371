"""`spmv-cache-trace-hip --compact[=round|exact]` without a GPU: every combination it cannot run is refused while the options are
parsed (argp: exit status 64, one line naming the reason), and without a usable device it fails instead of running anything in
its place."""
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
    (["--csr", BUS, "--compact", "--symmetric"], "cannot be combined with --symmetric"),
    (["--spmv-format", "hip-csr", "-m", "synthetic:queen:4,4,4:tril", "--symmetric", "--compact=exact"], "cannot be combined with --symmetric"),
    (["--csr", GENERAL, "--compact", "--transpose"], "cannot be combined with --transpose"),
    (["--csr", GENERAL, "--compact=round", "--vectors", "4"], "cannot be combined with --vectors"),
    (["--csr", GENERAL, "--compact", "--f32-values"], "cannot be combined with --f32-values"),
    (["--csr", GENERAL, "--f32-values=exact", "--compact=exact"], "cannot be combined with --f32-values"),
    (["--csr", GENERAL, "--compact", "--gpus", "2"], "--gpus must be 1"),
    (["--spmv-format", "hip-csr", "-m", "synthetic:queen:4,4,4", "--compact", "--gpus", "4"], "runs on one device"),
    (["--spmv-format", "csr", "-m", GENERAL, "--compact"], "no CPU kernel over 16-bit column codes"),
    (["--csr", GENERAL, "--device", "cpu", "--compact"], "no CPU kernel over 16-bit column codes"),
    (["--spmv-format", "coo", "-m", GENERAL, "--compact"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-coo", "-m", GENERAL, "--compact"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-ell", "-m", GENERAL, "--compact"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-hybrid", "-m", GENERAL, "--compact"], "needs the CSR kernel on the GPU"),
    (["--coo", GENERAL, "--compact"], "needs the CSR kernel on the GPU"),
    (["--ell", GENERAL, "--compact"], "needs the CSR kernel on the GPU"),
    (["--compact", "--triad", "1000"], "needs the CSR kernel on the GPU"),
])
def test_refused_while_parsing(args, message):
    r = _run(args)
    assert r.returncode == 64, (r.returncode, r.stderr)
    assert message in r.stderr, r.stderr
    assert "--compact" in r.stderr
    assert r.stdout == ""


def test_an_unknown_mode_is_refused_while_parsing():
    r = _run(["--csr", GENERAL, "--compact=nearest"])
    assert r.returncode == 64 and "expected 'round' (the default) or 'exact'" in r.stderr and r.stdout == ""


def test_accepted_combinations_pass_the_parser():
    """What --compact is for gets past the option checks (it then needs a device: see below)."""
    for args in (["--csr", GENERAL, "--compact"], ["--spmv-format", "hip-csr", "-m", GENERAL, "--compact=round"],
                 ["--csr", "synthetic:queen:4,4,4", "--compact=exact", "--gpus", "1"], ["--device", "hip", "--csr", BUS, "--compact"],
                 ["--csr", BUS, "--compact", "--expand-symmetric", "--check", "--x", "uniform"],
                 ["--csr", GENERAL, "--compact", "--exact-order"]):
        r = _run(args)
        assert r.returncode != 64, (args, r.stderr)


def test_without_a_device_it_fails_and_does_not_fall_back():
    from spmv_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present: this covers the box without one")
    for args in (["--csr", GENERAL, "--compact"], ["--spmv-format", "hip-csr", "-m", GENERAL, "--compact=exact"],
                 ["--csr", "synthetic:queen:4,4,4", "--compact", "--check"]):
        r = _run(args)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert r.stdout == "", r.stdout  # no JSON document: nothing ran
        assert "no CPU" in r.stderr or "no HIP device" in r.stderr, r.stderr
        assert "the CPU (OpenMP) kernel runs" not in r.stderr
    # SPMV_DEVICE=cpu cannot make it run on the CPU either
    r = _run(["--csr", GENERAL, "--compact"], env={"SPMV_DEVICE": "cpu"})
    assert r.returncode == 1 and r.stdout == "" and "no CPU kernel over 16-bit column codes" in r.stderr


def test_help_names_the_option():
    r = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "--compact" in r.stdout and "16-bit" in r.stdout
