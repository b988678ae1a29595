"""The device kd-tree layout (my-mitsuba_amd/csrc/kd_layout.h) is host code:
tools/check_kd_layout.cpp runs it on the Cornell box, on a builder scene of 2
rectangles and 12 triangles under a hand-made tree
(tests/golden/leaf_filter_scene.txt: leaves of rectangle records only, with a
rectangle record first, in the middle and last) and on one-leaf trees (the kd
root a leaf).  It holds the unfiltered arrays to the bytes the library
uploaded before the layout moved into the header
(tests/golden/kd_layout_cbox_digests.txt, FNV-1a 64 recorded from that commit)
and the filtered leaf addressing to its definition: the same blocks and inner
words, every filtered range the original one minus its MTSG_TRIACCEL_SHAPE
records in order, untouched leaves unchanged, every range inside triL.  `make`
builds it with ASan + UBSan; no GPU is involved."""
import os
import subprocess

from conftest import REPO


def test_kd_layout_under_sanitizers():
    exe = os.path.join(REPO, "tools", "check_kd_layout")
    subprocess.check_call(["make", "-C", REPO, "tools/check_kd_layout"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe, REPO], capture_output=True, text=True, cwd=REPO, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert "check_kd_layout: ok" in r.stdout
