"""tests/mount_ref.py -- the NumPy restatement of the mounted fan (include/pcp_abi.h) -- on the
CPU: at zero tilt its march is the oracle's, a beam table filled by the uniform formula changes
nothing, the sign convention of pitch and roll is checked against plain geometry, every blocked
ray's query point has a point within r and the sample before it has none, and the directions are
pcp_fan_dir.hpp's bit for bit (tests/native/fan_dir_selftest.cpp, built with the host compiler)."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import mount_ref
import numpy as np
import pytest
import scan_ref

from pointcloud_processor_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pointcloud_processor_amd" / "csrc"
SHAPES = [(100, 37, 15.0), (64, 3, 110.0)]


def _level6(poses5):
    p = np.asarray(poses5, np.float64)
    z = np.zeros(p.shape[0])
    return np.ascontiguousarray(np.column_stack([p[:, :3], z, z, p[:, 4]]))


def _uniform_table(fan):
    return np.array([fan.el_min + (fan.el_max - fan.el_min) * (float(j) + 0.5) / float(fan.n_el)
                     for j in range(fan.n_el)], np.float64)


@pytest.mark.parametrize("n_az,n_el,dmax", SHAPES)
def test_zero_tilt_is_the_oracles_march(oracle, n_az, n_el, dmax):
    cloud, poses5, fan, fh, blocked, _ = scan_ref.clutter_case(oracle, n_az, n_el, dmax)
    mfh, mb, mu = mount_ref.mount_case(("level", n_az, n_el, dmax), cloud, _level6(poses5), fan)[:3]
    np.testing.assert_array_equal(mfh, fh)
    np.testing.assert_array_equal(mb, blocked)
    _, units, _ = oracle.raycast_fan(oracle.Cloud(cloud), poses5, n_az, n_el, fan.el_min,
                                     fan.el_max, fan.max_distance)
    np.testing.assert_array_equal(mu, units)
    assert int(mb.sum()) > 0


@pytest.mark.parametrize("n_az,n_el,dmax", SHAPES)
def test_uniform_formula_as_a_table(oracle, n_az, n_el, dmax):
    cloud, poses5, fan, fh, blocked, _ = scan_ref.clutter_case(oracle, n_az, n_el, dmax)
    tab = _uniform_table(fan)
    p6 = _level6(poses5)
    d0 = mount_ref.directions(p6, fan)
    d1 = mount_ref.directions(p6, fan, tab)
    assert d0.tobytes() == d1.tobytes()
    tfh, tb, _ = mount_ref.first_hits(cloud, p6, fan, tab)
    np.testing.assert_array_equal(tfh, fh)
    np.testing.assert_array_equal(tb, blocked)


def _slab():
    """Points at xy pitch 0.05 m in the layers z = 0, -0.05, -0.10, -0.15, x and y in [-7, 7]."""
    g = np.arange(-140, 141) * 0.05
    x, y, z = np.meshgrid(g, g, np.array([0.0, -0.05, -0.10, -0.15]), indexing="ij")
    c = np.zeros((x.size, 4), np.float32)
    c[:, 0], c[:, 1], c[:, 2] = x.ravel(), y.ravel(), z.ravel()
    return c


def test_sign_convention_against_geometry():
    """Pitch -0.4363 from 2 m up looks down: the forward ray meets the slab near 2 / sin 0.4363 =
    4.73 m.  A sample needs z <= 0.056 to be within r of the slab, and the first sample that is
    >= 0.127 m lower lies inside it, where the nearest point is at most sqrt(0.0354^2 + 0.025^2) =
    0.043 m < r away: the hit depth lies in [4.60, 5.20).  The backward ray rises: no return.
    Roll +0.3 instead: the +y ray rises and the -y ray descends."""
    cloud = _slab()
    fan = _abi.FanParams(4, 1, 0.0, 0.0, 15.0)
    steps = scan_ref.step_table(fan.max_distance - mount_ref.KVIS)
    pose = np.array([[0.0, 0.0, 2.0, 0.0, -0.4363, 0.0]])
    fh, blocked, units = mount_ref.first_hits(cloud, pose, fan, [0.0])
    k = int(fh[0, 0, 0])
    assert k >= 0 and 4.60 <= steps[k] < 5.20
    assert fh[0, 0, 2] == -1
    d = mount_ref.directions(pose, fan, [0.0])[0, 0]
    assert d[0, 2] < -0.4 and d[2, 2] > 0.4 and abs(d[1, 2]) < 1e-12 and abs(d[3, 2]) < 1e-12
    assert blocked[0] == np.count_nonzero(fh >= 0)
    assert units[0] == sum(int(v) + 1 if v >= 0 else steps.size for v in fh.ravel())
    roll = np.array([[0.0, 0.0, 2.0, 0.3, 0.0, 0.0]])
    d = mount_ref.directions(roll, fan, [0.0])[0, 0]
    assert d[1, 2] > 0.29 and d[3, 2] < -0.29 and d[1, 1] > 0.9 and d[3, 1] < -0.9
    fh, _, _ = mount_ref.first_hits(cloud, roll, fan, [0.0])
    assert fh[0, 0, 1] == -1 and fh[0, 0, 3] >= 0
    assert 2.0 / np.sin(0.3) - 0.3 <= steps[int(fh[0, 0, 3])] < 2.0 / np.sin(0.3) + 0.6


@pytest.mark.parametrize("n_az,n_el,dmax", SHAPES)
def test_blocked_samples_have_a_point_and_the_ones_before_none(oracle, n_az, n_el, dmax):
    cloud = scan_ref.clutter_cloud()
    fan = _abi.fan_params(n_az=n_az, n_el=n_el, max_distance=dmax)
    fh, blocked, units, ref = mount_ref.mount_case(("clutter", n_az, n_el, dmax), cloud,
                                                   mount_ref.clutter_poses6(), fan)
    T = oracle.Cloud(cloud)
    q, qprev, k = ref["q"], ref["qprev"], ref["k"]
    M = q.shape[0]
    assert M == int(blocked.sum()) > 0
    r = scan_ref.RAY_RADIUS
    stride = max(1, M // 4000)
    for m in range(0, M, stride):
        assert T.count_within(q[m], r) > 0, m
        if k[m] > 0:
            assert T.count_within(qprev[m], r) == 0, m
    # a sample of an unblocked ray has none either (a few rays, every sample)
    steps = scan_ref.step_table(dmax - mount_ref.KVIS)
    p6 = mount_ref.clutter_poses6()
    d = mount_ref.directions(p6, fan)
    free = np.argwhere(fh < 0)
    for p, j, i in free[:: max(1, free.shape[0] // 12)]:
        for s in steps:
            qq = mount_ref.sample_points(p6[p:p + 1], d[p:p + 1, j, i], s)[0]
            assert T.count_within(qq, r) == 0, (p, j, i, s)


@pytest.fixture(scope="module")
def selftest_lines(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("fan_dir") / "fan_dir_selftest"
    # -fno-builtin: the definition's cos and sin are libm's two functions; g++ would otherwise
    # merge the pair of one argument into sincos, whose results differ from theirs in rare last bits
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-fno-builtin", f"-I{CSRC}",
                    str(ROOT / "tests" / "native" / "fan_dir_selftest.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr)
    return r.stdout.splitlines()


def _dbl(h):
    return struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0]


def test_directions_are_the_headers_bit_for_bit(selftest_lines):
    poses, fans, got = {}, {}, {}
    for ln in selftest_lines:
        w = ln.split()
        if w[0] == "pose":
            poses[int(w[1])] = [_dbl(h) for h in w[2:8]]
        elif w[0] == "fan":
            n = int(w[6])
            fans[int(w[1])] = (int(w[2]), int(w[3]), _dbl(w[4]), _dbl(w[5]),
                               [_dbl(h) for h in w[7:7 + n]])
        elif w[0] == "dir":
            c, p, i, j = map(int, w[1:5])
            got.setdefault(c, {})[(p, j, i)] = tuple(int(h, 16) for h in w[5:8])
    assert len(poses) == 10 and len(fans) == 4
    p6 = np.array([poses[p] for p in sorted(poses)])
    compared = 0
    for c, (n_az, n_el, el_min, el_max, table) in fans.items():
        fan = _abi.FanParams(n_az, n_el, el_min, el_max, 15.0)
        d = mount_ref.directions(p6, fan, table if table else None)
        bits = np.ascontiguousarray(d).view(np.uint64)
        assert len(got[c]) == p6.shape[0] * n_el * n_az
        for (p, j, i), b in got[c].items():
            assert tuple(int(v) for v in bits[p, j, i]) == b, (c, p, j, i)
            compared += 1
    assert compared == 10 * (3700 + 192 + 35 + 4)
