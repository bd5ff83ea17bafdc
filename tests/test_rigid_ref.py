"""rigid_ref.py on the CPU: the float64 reference is a rotation, the float32 numpy restatement
of make_rigid + xform_pt is the oracle's transform bit for bit, and the inputs of
test_rigid_gpu.py can tell a wrong kernel from a right one -- four wrong versions of the
restatement (a flipped sign of twx, m12 / m21 transposed, the third product fused, the sum
associated the other way) all differ from the oracle under the `tilt` quaternion, and none of
them does under the yaw that the suite's transforms used before: with q.x = q.y = 0 the entries
they touch are zero.  Two facts of the oracles that the GPU tests lean on close the file: q and
-q give the same bytes everywhere, and the carve's tf2 matrix is the same for q and 2 q."""
import math

import numpy as np
import pytest

import rigid_ref as rr
from test_filter_plan_gpu import _tfs

RGB = (1, 2, 3)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def cloud():
    c = rr.cloud()
    c.flags.writeable = False
    return c


def test_the_list():
    """The quaternions are what their names say."""
    q = rr.QUATS
    assert set(q) == {"tilt", "neg_w", "near_pi", "non_unit_small", "non_unit_big", "zero",
                      "gimbal"}
    assert all(abs(c) > 0.03 for c in q["tilt"]) and q["tilt"][3] > 0
    assert q["neg_w"] == tuple(-c for c in q["tilt"]) and q["neg_w"][3] < 0
    for name in rr.UNIT:
        assert abs(math.fsum(c * c for c in q[name]) - 1.0) < 4e-16
    assert abs(2.0 * math.degrees(math.acos(q["near_pi"][3])) - 179.9) < 1e-9
    x, y, z, _ = q["near_pi"]
    assert abs(y / x - 2.0) < 1e-12 and abs(z / x - 3.0) < 1e-12
    for name, s in (("non_unit_small", 0.6), ("non_unit_big", 1.7)):
        assert abs(math.sqrt(math.fsum(c * c for c in q[name])) - s) < 1e-15
    # gimbal: tf2's setRotation gives m[2][0] = xz - wy = -1 exactly
    qx, qy, qz, qw = q["gimbal"]
    s = 2.0 / (qx * qx + qy * qy + qz * qz + qw * qw)
    assert qx * (qz * s) - qw * (qy * s) == -1.0
    for t in [rr.T_TILT] + [rr.translation(i) for i in range(9)]:
        assert all(float(np.float32(c)) != c for c in t)


def test_reference_is_the_rotation():
    """apply() against the rotation built another way again: Rz(yaw) Ry(pitch) Rx(roll) as
    three float64 matrices for `tilt`, Rodrigues' formula for `near_pi`; lengths kept."""
    rng = np.random.default_rng(5)
    p = rng.uniform(-50, 50, (500, 3))
    r, pt, y = (math.radians(a) for a in (5.0, -8.0, 20.0))
    rx = np.array([[1, 0, 0], [0, math.cos(r), -math.sin(r)], [0, math.sin(r), math.cos(r)]])
    ry = np.array([[math.cos(pt), 0, math.sin(pt)], [0, 1, 0], [-math.sin(pt), 0, math.cos(pt)]])
    rz = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
    t = np.array(rr.T_TILT)
    want = p @ (rz @ ry @ rx).T + t
    for name in ("tilt", "neg_w"):
        np.testing.assert_allclose(rr.apply(p, t, rr.QUATS[name]), want, rtol=0, atol=1e-12)
    k = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    a = math.radians(179.9)
    want = p * math.cos(a) + np.cross(k, p) * math.sin(a) + \
        np.outer(p @ k, k) * (1 - math.cos(a)) + t
    got = rr.apply(p, t, rr.QUATS["near_pi"])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.linalg.norm(got - t, axis=1), np.linalg.norm(p, axis=1),
                               rtol=1e-14)


@pytest.mark.parametrize("name", list(rr.QUATS))
def test_restatement_is_the_oracle(oracle, cloud, name):
    """xform_f32 (no mutant) == oracle.transform_rgb bit for bit, and the colour word."""
    q, t = rr.QUATS[name], rr.T_TILT
    ref = oracle.transform_rgb(cloud, t, q, RGB)
    np.testing.assert_array_equal(_u32(rr.xform_f32(cloud, t, q)), _u32(ref[:, :3]))
    assert np.all(_u32(ref[:, 4]) == rr.colour_word(RGB)) and rr.colour_word(RGB) == 0xFF010203
    assert np.all(_u32(ref[:, 3]) == _u32(np.float32(1.0))) and not _u32(ref[:, 5:]).any()


@pytest.mark.parametrize("name", rr.UNIT)
def test_oracle_within_the_bound(oracle, cloud, name):
    q, t = rr.QUATS[name], rr.T_TILT
    worst = rr.units(oracle.transform_rgb(cloud, t, q, RGB), cloud, t, q)
    print(f"{name}: oracle within {worst:.2f} units of the bound")
    assert worst <= 1.0


@pytest.mark.parametrize("mutant", rr.MUTANTS)
def test_mutant_caught_under_tilt(oracle, cloud, mutant):
    """Every wrong version differs from the oracle on the GPU tests' `tilt` cloud; a wrong sign
    and a transposed entry also break the float64 bound."""
    q, t = rr.QUATS["tilt"], rr.T_TILT
    ref = oracle.transform_rgb(cloud, t, q, RGB)
    got = rr.xform_f32(cloud, t, q, mutant)
    differ = int((_u32(got) != _u32(ref[:, :3])).sum())
    worst = rr.units(got, cloud, t, q)
    print(f"{mutant}: {differ} of {got.size} words differ, {worst:.3g} units of the bound")
    assert differ >= 1
    if mutant in ("twx_sign", "m12_m21_swapped"):
        assert worst > 1.0


@pytest.mark.parametrize("mutant", rr.MUTANTS)
def test_mutant_missed_under_the_old_yaw(oracle, cloud, mutant):
    """Under the yaw of test_filter_plan_gpu._tfs() -- (0, 0, s, c), the shape of every rotation
    about z the suite fed the library -- twx, m12, m21 and each row's third product are zero:
    all four wrong versions give the oracle's bits.  This is why the new inputs exist."""
    t, q = _tfs(2)[1]
    assert q[0] == 0.0 and q[1] == 0.0 and q[2] != 0.0
    ref = oracle.transform_rgb(cloud, t, q, RGB)
    np.testing.assert_array_equal(_u32(rr.xform_f32(cloud, t, q, mutant)), _u32(ref[:, :3]))


@pytest.mark.parametrize("name", list(rr.QUATS))
def test_transform_of_minus_q(oracle, cloud, name):
    q = rr.QUATS[name]
    a = oracle.transform_rgb(cloud, rr.T_TILT, q, RGB)
    b = oracle.transform_rgb(cloud, rr.T_TILT, rr.scaled(q, -1.0), RGB)
    np.testing.assert_array_equal(_u32(a), _u32(b))


def test_drivable_of_minus_q(oracle):
    c = rr.drive_cloud()
    g0, o0 = rr.drive_oracle(oracle, c, rr.T_TILT, rr.QUATS["tilt"])
    g1, o1 = rr.drive_oracle(oracle, c, rr.T_TILT, rr.QUATS["neg_w"])
    assert {-1, 0, 100} <= set(np.unique(g0).tolist())
    np.testing.assert_array_equal(g0, g1)
    np.testing.assert_array_equal(o0.view(np.uint64), o1.view(np.uint64))


@pytest.mark.parametrize("other", ["neg_w", "twice"])
def test_excavate_of_minus_q_and_2q(oracle, other):
    """-q: every product of two components keeps its sign.  2 q: d is 4 d, s = 2 / d a quarter
    (exact: a power of two), each product the same double."""
    q = rr.QUATS["tilt"]
    q2 = rr.QUATS["neg_w"] if other == "neg_w" else rr.scaled(q, 2.0)
    ref, got = rr.carve_reference(oracle, q), rr.carve_reference(oracle, q2)
    assert 0 < ref[0].sum() < ref[0].size
    for a, b in zip(ref, got):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
