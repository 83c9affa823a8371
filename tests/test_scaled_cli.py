"""--alpha / --beta of the host program without a GPU: they are refused without a float-tile mode (--f32-values, --compact), a
value that is no number is refused, and on the CPU there is no kernel to scale.  The run on a device is in test_gpu_scaled.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spmv-cache-trace_amd", "spmv-cache-trace-hip")
BUS = os.path.join(ROOT, "tests", "golden", "bus1138_like.mtx")


def _run(*options):
    return subprocess.run([CLI, "--csr", BUS, "--threads", "1", "--profile", "2"] + list(options), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


@pytest.mark.parametrize("options", [["--alpha", "2"], ["--beta", "0"], ["--alpha", "-1", "--beta", "1", "--device", "cpu"],
                                     ["--alpha", "2", "--symmetric"], ["--beta", "0.5", "--transpose"], ["--alpha", "2", "--vectors", "4"]])
def test_alpha_and_beta_need_a_float_tile_mode(options):
    r = _run(*options)
    assert r.returncode != 0 and r.stdout == ""
    assert "--alpha / --beta need --f32-values or --compact[=f64|f32]" in r.stderr, r.stderr


@pytest.mark.parametrize("mode", ["--f32-values", "--compact", "--compact=f64", "--compact=f32"])
def test_alpha_that_is_no_number_is_refused(mode):
    for options in (["--alpha", "two"], ["--beta", "1x"], ["--alpha", ""]):
        r = _run(mode, *options)
        assert r.returncode != 0 and r.stdout == ""
        assert "expected a number" in r.stderr, r.stderr


@pytest.mark.parametrize("mode,what", [("--f32-values", "there is no CPU kernel over float values"),
                                       ("--compact", "there is no CPU kernel over 16-bit column codes"),
                                       ("--compact=f64", "there is no CPU kernel over 16-bit column codes"),
                                       ("--compact=f32", "there is no CPU kernel over 16-bit column codes")])
def test_on_the_cpu_there_is_no_kernel_to_scale(mode, what):
    r = _run(mode, "--alpha", "-1", "--beta", "1", "--device", "cpu")
    assert r.returncode != 0 and r.stdout == ""
    assert what in r.stderr and "unrecognized option" not in r.stderr, r.stderr


def test_help_names_both_options():
    r = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0
    assert "--alpha=A" in r.stdout and "--beta=B" in r.stdout
