"""The kernel registry (varpro_amd/csrc/vp_registry.hpp) from a plain host C++ program (tests/cpp/test_registry.cpp): what the
set builders guarantee about every registered kernel set, and a dump of every field of every set.  Needs no GPU."""
import os
import subprocess

from varpro_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "cpp", "test_registry")


def _run(*args):
    # (always: the program holds KernelEntry's layout; make rebuilds it when the header or the library is newer)
    subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-s", "test_registry"])
    out = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_cpp_registry_invariants_and_dump():
    assert " 0 failure(s)" in _run()
    lines = _run("--dump").splitlines()
    assert lines
    n = len(_lib.registry_entries())
    assert n > 0 and sum(line.startswith("registry[") for line in lines) == n
    assert [line.split(" ")[0] for line in lines[n:]] == ["generic[0]", "generic[1]", "external[0]", "external[1]"]
    # the two wrappers of the caller-evaluated sets are the only launchers without a dynamic symbol
    assert [line.count("=local") for line in lines] == [0] * (n + 2) + [1, 1]
