"""k_candidates / k_cand_compact (pcp_score.hip), through pcp_generate_candidates and
pcp_generate_and_score, on the scenes of tests/cand_cases.py: every branch of
generateCandidatePositions / getGroundHeight and every path of the two kernels and their host
code that the golden scene never takes -- several compaction chunks with a partial last one,
both landings (pinned up to 4 MiB, the device buffer past it), the fused tick past one chunk,
with a device-read count of 0 and its two-call fallback past 65,535 lattice points, the axis
cases of atan2, rows of 0 to 9 points, windows that miss the grid, negative and absent ground,
points on and next to the boundaries of the strict tests, queries 3 km from the origin.

The bar: the count and x, y, z bit-identical to the oracle AND to the brute-force reference
tests/cand_ref.py; pitch and yaw bit-identical to the reference (tests/cr_ref.py's correctly
rounded atan2, the IEEE special values on the axes), no allowance; against the oracle's glibc
angles at most one ulp, the number that differ printed.  tests/test_cand_ref.py proves the
reference right and the scenes biting.

Not reachable: the row loop's second stride (rows > 1,024 threads).  The index cell is at least
0.112 m, the window 2 (1 + m) m by 2 (2 + m) m, which gives at most about 19 x 37 = 703 rows.

Measured on an MI355X (ROCm 7.2), printed by each run:
  * every case bit-identical to the reference, 0 undecided; no kernel fault found;
  * angles that differ from glibc's (one ulp each): 0 in each of the 35 small cases (0 to 256
    poses), 2 of 8,096 in gs257, 95 of 156,816 in land_pinned, 120 of 157,464 in land_edge --
    6 to 8 in 10,000, so an allowance of 2 values cannot hold past a few thousand poses;
  * the axis results (dyadic9): every pitch -0x1.921fb54442d18p+0 (-pi / 2: elevation
    atan2(-0.0, hd) = -0.0); yaws atan2(+0.0, 4) = atan2(+0.0, 3) = 0x0.0p+0,
    atan2(4, 0) = atan2(3, 0) = 0x1.921fb54442d18p+0, atan2(-3, 0) = atan2(-4, 0) =
    -0x1.921fb54442d18p+0, atan2(+0.0, -3) = atan2(+0.0, -4) = 0x1.921fb54442d18p+1: the IEEE
    special values; ocml's raw atan2 returns them too (tests/test_device_math_gpu.py, the
    `axes` family: 0 of 1,024 not correctly rounded);
  * the sampled checks: 1,076 / 1,083 lattice points (809 / 812 valid) and 4,901 / 4,921 poses;
  * the whole module takes about 3 s."""
import ctypes as C
import math

import numpy as np
import pytest

import cand_cases
import cand_ref
from pointcloud_processor_amd import _abi, synth

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300


@pytest.fixture(scope="module")
def ctx():
    c = _abi.Context(0)
    yield c
    c.close()


def _params(c):
    return _abi.default_vl_params(search_radius=c["search_radius"],
                                  sensor_height=c["sensor_height"],
                                  num_candidates=c["num_candidates"])


def _set_terrain(ctx, c):
    """The case's terrain as PointXYZRGB records (an empty cloud: no ground query, as in the
    reference; the index of the cloud before stays, unused)."""
    ctx.set_terrain(synth._pack(c["terrain"], (255, 0, 0)), point_step=32)


def _generate(ctx, c):
    _set_terrain(ctx, c)
    return ctx.generate_candidates(c["bbox"], _params(c), c["zx"])


def _against_oracle(name, g, r):
    assert g.shape == r.shape
    assert g[:, :3].tobytes() == r[:, :3].tobytes()
    off = cand_ref.ulp_distance(g[:, 3:], r[:, 3:])
    print(f"{name}: {g.shape[0]} poses, {int((off > 0).sum())} of {off.size} angles differ "
          f"from glibc's")
    assert (off <= 1).all()


@pytest.mark.parametrize("name", list(cand_cases.small_cases()))
def test_case(ctx, oracle, name):
    c = cand_cases.cases()[name]
    g = _generate(ctx, c)
    ref, _, und = cand_cases.reference(name)
    assert und == 0
    _against_oracle(name, g, cand_cases.oracle_poses(oracle, c))
    assert g.shape == ref.shape
    assert g[:, :3].tobytes() == ref[:, :3].tobytes()
    bad = np.nonzero((g[:, 3:].view(np.uint64) != ref[:, 3:].view(np.uint64)).any(1))[0]
    assert bad.size == 0, (name, g[bad][:4], ref[bad][:4])


def test_axis_angles(ctx):
    """The device's results where an argument of atan2 is zero (dyadic9: dz == 0 everywhere,
    dx == 0 or dy == 0 at 8 lattice points): the IEEE special values."""
    c = cand_cases.cases()["dyadic9"]
    g = _generate(ctx, c)
    axis = (g[:, 0] == 2.0) | (g[:, 1] == 2.0)
    print("dyadic9 pitches:", sorted({float(v).hex() for v in g[:, 3]}),
          "axis yaws:", [(float(x), float(y), float(w).hex()) for x, y, w in g[axis][:, [0, 1, 4]]])
    assert axis.sum() == 8 and (g[:, 3] == -math.pi / 2).all()
    for x, y, yaw in g[axis][:, [0, 1, 4]]:
        want = math.atan2(2.0 - y, 2.0 - x)
        assert np.float64(yaw).tobytes() == np.float64(want).tobytes(), (x, y, yaw, want)


@pytest.mark.parametrize("name", ["land_pinned", "land_edge"])
def test_landings(ctx, oracle, name):
    """323^2 lattice points land in pinned memory, 324^2 in a device buffer (the count read
    first, then the poses copied): in full against the oracle, every 97th lattice point's ground
    and every 16th pose's angles against the reference."""
    c = cand_cases.cases()[name]
    L = math.ceil(math.sqrt(c["num_candidates"])) ** 2
    assert (L * 40 + 4 > 4 << 20) == (name == "land_edge")
    g = _generate(ctx, c)
    _against_oracle(name, g, cand_cases.oracle_poses(oracle, c))
    lat = cand_ref.Lattice(c["terrain"], c["bbox"], c, c["zx"])
    n_l, n_valid, n_p, und = cand_ref.check_sampled(lat, g, cand_cases.SAMPLE_LATTICE,
                                                    cand_cases.SAMPLE_POSES)
    print(f"{name}: {n_l} lattice points ({n_valid} valid) and {n_p} poses against the reference")
    assert und == 0 and n_valid > 0.7 * n_l


def _raw_generate(ctx, c, cap, rows=None):
    """pcp_generate_candidates through the library itself into a sentinel-filled buffer ->
    (rc, n_out, buffer)."""
    buf = np.full((max(cap if rows is None else rows, 1), 5), SENTINEL, np.float64)
    bb = np.ascontiguousarray(c["bbox"], np.float64)
    zx = np.ascontiguousarray(c["zx"], np.float64)
    p = _params(c)
    n = C.c_uint64(12345)
    rc = ctx.lib.pcp_generate_candidates(ctx.h, _abi._ptr(bb), C.byref(p), _abi._ptr(zx),
                                         _abi._ptr(buf), cap, C.byref(n))
    return rc, n.value, buf


@pytest.mark.parametrize("name", ["gs33", "land_edge"])
def test_capacity(ctx, name):
    """A capacity one below the count, on both landings: PCP_E_CAPACITY, the needed count in
    *n_out, the caller's buffer untouched; a capacity equal to the count succeeds."""
    c = cand_cases.cases()[name]
    g = _generate(ctx, c)
    n = g.shape[0]
    assert n > 1
    for cap in (n - 1, 1):
        rc, need, buf = _raw_generate(ctx, c, cap, rows=n)
        assert rc == _abi.PCP_E_CAPACITY and need == n
        assert (buf == SENTINEL).all()
    rc, need, buf = _raw_generate(ctx, c, n)
    assert rc == _abi.PCP_OK and need == n and buf.tobytes() == g.tobytes()


def test_lattice_side_limit(ctx):
    """num_candidates = 4097^2 (a lattice side above 4,096): PCP_E_INVALID before anything is
    launched or allocated; 0 candidates: no lattice, 0 poses."""
    c = dict(cand_cases.cases()["dyadic9"], num_candidates=4097 * 4097)
    rc, n, buf = _raw_generate(ctx, c, 1)
    assert rc == _abi.PCP_E_INVALID and n == 0 and (buf == SENTINEL).all()
    rc, n, buf = _raw_generate(ctx, cand_cases.cases()["nc0"], 1)
    assert rc == _abi.PCP_OK and n == 0 and (buf == SENTINEL).all()


def _cells():
    """64 cells on the floor of the gs33 / gs65 boxes' near corner, normals up."""
    g = np.arange(8) * 0.5 + 0.25
    X, Y = np.meshgrid(g, g)
    xyz = np.stack([X.ravel(), Y.ravel(), np.full(64, 0.05)], 1)
    return xyz, np.tile(np.array([0.0, 0.0, 1.0], np.float32), (64, 1))


@pytest.mark.parametrize("name", ["gs33", "gs65_r0", "gs257"])
def test_generate_and_score_matches_two_calls(ctx, name):
    """pcp_generate_and_score against pcp_generate_candidates + pcp_score_poses on the same
    context, bit for bit: gs33 (fused, two compaction chunks, the host's pinned mirror), gs65
    with radius 0 (a device-read count of 0) and gs 257 (66,049 lattice points: the two-call
    fallback), over 64 cells, twice each (the flags carry over)."""
    c = cand_cases.cases()[name]
    xyz, nrm = _cells()
    ctx.set_cells(xyz, nrm)
    zx = np.array([-3.0, -3.0, 2.0, -0.5, 0.7])
    p = _params(c)
    try:
        _set_terrain(ctx, c)
        fa = np.zeros(64, np.uint8)
        fb = fa.copy()
        for _ in range(2):
            poses = ctx.generate_candidates(c["bbox"], p, zx)
            tot, cov, rep = ctx.score_poses(poses, zx, p, fa)
            p2, tot2, cov2, rep2 = ctx.generate_and_score(c["bbox"], p, zx, fb)
            assert p2.shape == poses.shape and p2.tobytes() == poses.tobytes()
            assert tot2.tobytes() == tot.tobytes() and cov2.tobytes() == cov.tobytes()
            assert fb.tobytes() == fa.tobytes() and rep2.as_dict() == rep.as_dict()
        ref, _, _ = cand_cases.reference(name)
        assert poses.shape == ref.shape and poses[:, :3].tobytes() == ref[:, :3].tobytes()
        print(f"{name}: {poses.shape[0]} poses, {int((cov > 0).sum())} of them see a cell")
    finally:
        ctx.set_cells(np.zeros((0, 3)), np.zeros((0, 3), np.float32))


def test_no_stale_state(ctx):
    """A case run again after other terrains and lattices -- larger and smaller, both landings,
    an empty cloud -- gives identical bytes: nothing of the lattice buffer, the pinned landing
    or the index of the calls between survives into it."""
    first = {}
    order = ["nd10_dense", "gs65", "dyadic9", "far_boundaries", "gs33", "nd10_sparse", "gs2",
             "nd10_dense", "gs65", "far_boundaries", "gs33"]
    for name in order:
        g = _generate(ctx, cand_cases.cases()[name])
        if name in first:
            assert g.tobytes() == first[name].tobytes(), name
        first.setdefault(name, g)
