"""The example program with loads_every = 1 on the MI355X: build/bimocq3d with a paddle turning at +1 rad
per time unit in rising smoke prints one `loads` line per frame whose numbers parse and whose shaft torque opposes the spin."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 4


def test_example_prints_the_paddle_torque(tmp_path):
    exe = os.path.join(ROOT, "build", "bimocq3d")
    assert os.path.exists(exe), "build/bimocq3d missing: run `make`"
    cmd = [exe, "32", str(FRAMES), str(tmp_path), "0", "0", "0", "0", "0", "0", "0", "0", "1.0", "0", "1"]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("loads ")]
    assert len(lines) == FRAMES, r.stdout[-3000:]
    for f, w in enumerate(lines):
        assert w[:2] == ["loads", "frame"] and int(w[2]) == f and w[3] == "obstacle" and int(w[4]) == 0
        assert w[5] == "force" and w[9] == "torque" and w[13] == "area" and len(w) == 15
        force, torque, area = [float(x) for x in w[6:9]], [float(x) for x in w[10:13]], float(w[14])
        assert all(x == x and abs(x) < 1e30 for x in force + torque) and area > 0.0
        assert torque[2] < 0.0, (f, torque)
