"""--dots of the host program without a GPU: it is refused without --alpha / --beta and without a float-tile mode, as --alpha is,
and the help text lists it.  The run on a device is in test_gpu_dots.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spmv-cache-trace_amd", "spmv-cache-trace-hip")
BUS = os.path.join(ROOT, "tests", "golden", "bus1138_like.mtx")


def _run(*options):
    return subprocess.run([CLI, "--csr", BUS, "--threads", "1", "--profile", "2"] + list(options), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


@pytest.mark.parametrize("options", [["--dots"], ["--dots", "--compact"], ["--dots", "--f32-values"], ["--dots", "--compact=f64"],
                                     ["--dots", "--compact=f32"], ["--dots", "--device", "cpu"], ["--dots", "--symmetric"],
                                     ["--dots", "--alpha", "2"], ["--dots", "--beta", "0", "--transpose"]])
def test_dots_need_alpha_or_beta_and_a_float_tile_mode(options):
    r = _run(*options)
    assert r.returncode != 0 and r.stdout == ""
    assert "--dots needs --alpha / --beta and --f32-values or --compact[=f64|f32]" in r.stderr, r.stderr


def test_on_the_cpu_there_is_no_kernel_with_dots():
    r = _run("--compact=f64", "--alpha", "-1", "--beta", "1", "--dots", "--device", "cpu")
    assert r.returncode != 0 and r.stdout == ""
    assert "there is no CPU kernel over 16-bit column codes" in r.stderr and "unrecognized option" not in r.stderr, r.stderr


def test_help_lists_the_option():
    r = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0
    assert "--dots" in r.stdout and "spmv_hip_run_scaled_dots" in r.stdout
