"""The launchers' argument fillers (varpro_amd/csrc: fill_fit_args, fill_eval_args, lm_opts_from) and padding_variant from a
host C++ program (tests/cpp/test_launch_args.cpp): every field of a filled kernel argument record against a table, no byte of
it left unwritten, and the padding-variant rule against its three inequalities.  Launches nothing, needs no GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "cpp", "test_launch_args")


def test_cpp_launch_args():
    # (always: the program holds the records' layout; make rebuilds it when a header it includes is newer)
    subprocess.check_call(["make", "-C", os.path.join(HERE, "cpp"), "-s", "test_launch_args"])
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines()[-1] == "0 failure(s)", out.stdout
