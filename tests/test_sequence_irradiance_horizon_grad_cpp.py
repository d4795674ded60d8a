"""SunskySequence's irradiance gradients under a horizon profile through the C++ facade
(include/sunsky_amd.hpp), driven by a compiled stand-alone program,
tests/cpp/sequence_irradiance_horizon_grad_check.cpp, in host mode: irradiance_horizon_vjp compiles
against the header and refuses in the same places as the C ABI, as a C++ renderer linking
libsunsky_amd.so sees it.  The test compiles the program itself (one translation unit against the
built library)."""
import os
import shutil
import subprocess

import pytest

import sunsky_amd as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ to build the sequence irradiance horizon gradient check")
    out = str(tmp_path_factory.mktemp("sequence_irradiance_horizon_grad_check") / "sequence_irradiance_horizon_grad_check")
    libdir = os.path.dirname(ss.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROCM, "include"), "-o", out,
           os.path.join(ROOT, "tests", "cpp", "sequence_irradiance_horizon_grad_check.cpp"),
           "-L" + libdir, "-lsunsky_amd", "-Wl,-rpath," + libdir,
           "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def test_sequence_irradiance_horizon_grad_facade_host_mode(exe):
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sequence irradiance horizon grad host ok" in r.stdout
    assert "FAILED" not in r.stdout
    assert "sunsky_sequence_prepare_irradiance first" in r.stdout
    assert "sunsky_sequence_prepare_irradiance_grad first" in r.stdout
    assert "n_sectors" in r.stdout
    assert "host-only sequence" in r.stdout
