"""`spmv-cache-trace-hip --compact=f32` without a GPU: every combination it cannot run is refused while the options are parsed
(argp: exit status 64, one line naming the reason), and without a usable device it fails instead of running anything in its
place.  Children that must not find a device are started with none visible to them, so the tests mean the same on a box
with a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spmv-cache-trace_amd", "spmv-cache-trace-hip")
BUS = os.path.join(ROOT, "tests", "golden", "bus1138_like.mtx")          # `symmetric` header
GENERAL = os.path.join(ROOT, "tests", "golden", "poisson2D.mtx")        # `general` header


HIDDEN = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}  # no device for a child, whatever the box has


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("SPMV_DEVICE", None)
    if env:
        e.update(env)
    return subprocess.run([CLI] + args + ["--threads", "1", "--profile", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120, env=e)


@pytest.mark.parametrize("args, message", [
    (["--csr", BUS, "--compact=f32", "--symmetric"], "cannot be combined with --symmetric"),
    (["--spmv-format", "hip-csr", "-m", "synthetic:queen:4,4,4:tril", "--symmetric", "--compact=f32"], "cannot be combined with --symmetric"),
    (["--csr", GENERAL, "--compact=f32", "--transpose"], "cannot be combined with --transpose"),
    (["--csr", GENERAL, "--compact=f32", "--vectors", "4"], "cannot be combined with --vectors"),
    (["--csr", GENERAL, "--compact=f32", "--f32-values"], "--compact cannot be combined with --f32-values"),
    (["--csr", GENERAL, "--f32-values=exact", "--compact=f32"], "--compact stores the values as floats already"),
    (["--csr", GENERAL, "--compact=f32", "--gpus", "2"], "--gpus must be 1"),
    (["--spmv-format", "hip-csr", "-m", "synthetic:queen:4,4,4", "--compact=f32", "--gpus", "4"], "runs on one device"),
    (["--spmv-format", "csr", "-m", GENERAL, "--compact=f32"], "no CPU kernel over 16-bit column codes"),
    (["--csr", GENERAL, "--device", "cpu", "--compact=f32"], "no CPU kernel over 16-bit column codes"),
    (["--spmv-format", "coo", "-m", GENERAL, "--compact=f32"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-coo", "-m", GENERAL, "--compact=f32"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-ell", "-m", GENERAL, "--compact=f32"], "needs the CSR kernel on the GPU"),
    (["--spmv-format", "hip-hybrid", "-m", GENERAL, "--compact=f32"], "needs the CSR kernel on the GPU"),
    (["--coo", GENERAL, "--compact=f32"], "needs the CSR kernel on the GPU"),
    (["--ell", GENERAL, "--compact=f32"], "needs the CSR kernel on the GPU"),
    (["--compact=f32", "--triad", "1000"], "needs the CSR kernel on the GPU"),
])
def test_refused_while_parsing(args, message):
    r = _run(args)
    assert r.returncode == 64, (r.returncode, r.stderr)
    assert message in r.stderr, r.stderr
    assert "--compact" in r.stderr
    assert r.stdout == ""


def test_the_other_modes_keep_their_meaning():
    r = _run(["--csr", GENERAL, "--compact=nearest"])
    assert r.returncode == 64 and "expected 'round' (the default) or 'exact'" in r.stderr and "'f64'" in r.stderr and "'f32'" in r.stderr
    assert r.stdout == ""
    # --compact=f64 still says that IT multiplies doubles
    r = _run(["--csr", GENERAL, "--compact=f64", "--f32-values"])
    assert r.returncode == 64 and "--compact=f64 cannot be combined with --f32-values" in r.stderr


def test_accepted_combinations_pass_the_parser():
    for args in (["--csr", GENERAL, "--compact=f32"], ["--spmv-format", "hip-csr", "-m", GENERAL, "--compact=f32"],
                 ["--csr", "synthetic:queen:4,4,4", "--compact=f32", "--gpus", "1"], ["--device", "hip", "--csr", BUS, "--compact=f32"],
                 ["--csr", BUS, "--compact=f32", "--expand-symmetric", "--check", "--x", "uniform"],
                 ["--csr", GENERAL, "--compact=f32", "--exact-order"]):
        r = _run(args, env=HIDDEN)  # (it then needs a device: see below)
        assert r.returncode != 64, (args, r.stderr)


def test_without_a_device_it_fails_and_does_not_fall_back():
    for args in (["--csr", GENERAL, "--compact=f32"], ["--spmv-format", "hip-csr", "-m", GENERAL, "--compact=f32"],
                 ["--csr", "synthetic:queen:4,4,4", "--compact=f32", "--check"]):
        r = _run(args, env=HIDDEN)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert r.stdout == "", r.stdout  # no JSON document: nothing ran
        assert "no CPU" in r.stderr or "no HIP device" in r.stderr, r.stderr
        assert "the CPU (OpenMP) kernel runs" not in r.stderr
    # SPMV_DEVICE=cpu cannot make it run on the CPU either
    r = _run(["--csr", GENERAL, "--compact=f32"], env={"SPMV_DEVICE": "cpu"})
    assert r.returncode == 1 and r.stdout == "" and "no CPU kernel over 16-bit column codes" in r.stderr


def test_help_names_the_mode():
    r = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "round|exact|f64|f32" in r.stdout and "hip-csr-spmv-compact-f32" in r.stdout
