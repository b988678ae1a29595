"""The batch plan of a render call (my-mitsuba_amd/csrc/render_plan.h) is
integer arithmetic on the host: tools/check_render_plan.cpp sweeps rectangles,
sample counts, tile deals, key lists, lane counts and path budgets, checks that
every plan covers each (tile, sample) pair once within a lane's share of the
budget, and pins a few literal plans (README's "C5 in three batches").  `make`
builds it with ASan + UBSan; no GPU is involved."""
import os
import subprocess

from conftest import REPO


def test_render_plan_sweep_under_sanitizers():
    exe = os.path.join(REPO, "tools", "check_render_plan")
    subprocess.check_call(["make", "-C", REPO, "tools/check_render_plan"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, cwd=REPO, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert "plans ok" in r.stdout
