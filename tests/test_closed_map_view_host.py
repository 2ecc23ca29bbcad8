"""The host arithmetic of the view gain (tloam_amd/csrc/tl_view_box.hpp) under the host sanitizers,
without a GPU: a stand-alone program (tests/host/view_box_main.cpp, its own main, no HIP) built with
-fsanitize=address,undefined and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_view_arithmetic_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "view_box")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "view_box_main.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stderr == ""
    word, checks = run.stdout.split()
    assert word == "ok" and int(checks) > 500
