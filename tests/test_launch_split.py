"""The launch plans of vg_amd/csrc/launch_split.hpp — which item runs in which of a call's two launches, and which slice of the slab a large item
owns — run without a GPU: tests/emu/launch_split_san_main.cpp holds them to a brute force of its own under the host sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_plans_under_the_host_sanitizers():
    """a program of its own under -fsanitize=address,undefined, nothing preloaded: every statement holds, nothing reported"""
    subprocess.check_call(["make", "-s", "launch_split_san"], cwd=ROOT)
    done = subprocess.run([os.path.join(ROOT, "tests", "emu", "launch_split_san")], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stderr[-2000:]
