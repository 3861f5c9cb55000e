"""csrc/hdg_cg_pending.hpp on the CPU: the queue of deferred p / x updates of the condensed CG (plain C++, no HIP)."""
import os
import shutil
import subprocess

import pytest


def test_pending_cg_updates_are_applied_once_in_order_from_live_slots(tmp_path):
    """tests/host/cg_pending_check.cpp, compiled with g++ -fsanitize=address,undefined and run: for every ring size M <= 8, every
    iteration count <= 40, every position of a forced flush and both kinds of exit, every update is applied exactly once and in
    order from a slot that still holds its z, no queued slot is overwritten, and only a normal exit drops the newest update.
    8 * (2 + ... + 41) * 2 = 13 760 cases."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "cg_pending_check"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "cg_pending_check.cpp")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), src], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 13760", r.stdout + r.stderr
