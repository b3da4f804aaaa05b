"""Global-fit statistics (vp_global_statistics) from a plain-C caller (tests/c/test_global_statistics.c, gcc -std=c99
-pedantic) and from the C++ mirror (tests/cpp/test_global_statistics.cpp, varpro.hpp).  Both programs are compiled here,
into the test's temporary directory; the Makefiles of tests/c and tests/cpp are not involved."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBDIR = os.path.join(ROOT, "varpro_amd", "lib")


def _build_c(tmp):
    exe = os.path.join(str(tmp), "test_global_statistics_c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "c", "test_global_statistics.c"), "-o", exe, "-L" + LIBDIR, "-lvarpro_hip", "-lm",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _build_cpp(tmp):
    exe = os.path.join(str(tmp), "test_global_statistics_cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(HERE, "cpp", "test_global_statistics.cpp"),
                           "-o", exe, "-L" + LIBDIR, "-lvarpro_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_c_and_cpp_programs_build_and_refuse_without_parameters(tmp_path):
    for exe in (_build_c(tmp_path), _build_cpp(tmp_path)):
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "0 failure(s)" in out.stdout


@pytest.mark.gpu
def test_global_statistics_from_plain_c(tmp_path):
    out = subprocess.run([_build_c(tmp_path), "expect_gpu"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "global statistics from C: 0 failure(s)" in out.stdout


@pytest.mark.gpu
def test_global_statistics_from_the_cpp_mirror(tmp_path):
    out = subprocess.run([_build_cpp(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failure(s)" in out.stdout and "global fit:" in out.stdout
