"""tests/cand_ref.py -- the brute-force reference of generateCandidatePositions / getGroundHeight
that tests/test_candidates_gpu.py holds the device to -- is right, and the scenes of
tests/cand_cases.py bite.  CPU only.

Right: on every case the reference equals the oracle (oracle/pcp_oracle.c, its own grid walk,
glibc's atan2): the same count, x, y and z bit for bit, the angles within one ulp (glibc's rare
near-tie misroundings); no cr_atan2 call comes back undecided.

Bite: each mutation switch of cand_ref (a boundary made non-strict or strict, the 2-D distance
from the float query or with its sum rounded once, a maximum that starts at 0, a window without
margin, a block maximum of one wave, a row's tail dropped, a compaction that forgets its base)
changes the output of the case named for it in CAUGHT_BY; the reason codes show every rejection
hit, and hit on its boundary where one is constructed."""
import math

import numpy as np
import pytest

import cand_cases
import cand_ref

# mutation -> the case that must tell it from the reference
CAUGHT_BY = {
    "zx_le": "dyadic9",                  # two lattice points exactly 0.5 from zx120
    "flann_le": "dyadic9_boundaries",    # points at squared 3-D distance exactly 4.0f
    "d2_le": "dyadic9_boundaries",       # a point at 2-D distance exactly 1.0
    "box_strict": "dyadic9",             # lattice points on the box faces
    "d2_float_query": "nd10_boundaries", # distances a few ulps either side of 1.0
    "d2_fused": "fuse",                  # the unfused and the once-rounded sum disagree
    "max_init0": "nd10_sunk",            # negative ground
    "win_float": "far_boundaries",       # points 1 m from the float query, nearer the double
    "rows64": "nd10_dense",              # the highest point lies above the first 64 rows
    "tail4": "nd10_rows",                # rows of 1 .. 9 points, the highest last
    "chunk_base": "gs33",                # two compaction chunks
}

_ref = cand_cases.reference
_oracle = cand_cases.oracle_poses


@pytest.mark.parametrize("name", list(cand_cases.small_cases()))
def test_reference_equals_oracle(oracle, name):
    c = cand_cases.cases()[name]
    poses, reasons, und = _ref(name)
    r = _oracle(oracle, c)
    assert und == 0, f"{name}: {und} undecided -- change the case's numbers"
    assert len(reasons) == math.ceil(math.sqrt(c["num_candidates"])) ** 2
    assert poses.shape == r.shape and reasons.count("valid") == r.shape[0]
    assert poses[:, :3].tobytes() == r[:, :3].tobytes()
    off = cand_ref.ulp_distance(poses[:, 3:], r[:, 3:])
    print(f"{name}: {r.shape[0]} poses, glibc differs on {int((off > 0).sum())} angles")
    assert (off <= 1).all()


@pytest.mark.parametrize("name", [k for k, c in cand_cases.cases().items() if c["sampled"]])
def test_reference_equals_oracle_sampled(oracle, name):
    """The two large lattices: every 97th lattice point's ground and every 16th pose's angles
    (the oracle's poses within one ulp of them)."""
    c = cand_cases.cases()[name]
    r = _oracle(oracle, c)
    lat = cand_ref.Lattice(c["terrain"], c["bbox"], c, c["zx"])
    glibc = r.copy()
    rows = np.arange(0, r.shape[0], cand_cases.SAMPLE_POSES)
    for k in rows:   # the reference's angles into the sampled rows; the rest stays the oracle's
        elev, yaw, und = lat.angles(*(float(v) for v in r[k, :3]))
        assert und == 0
        r[k, 3:] = (-math.pi / 2 + elev, yaw)
    assert (cand_ref.ulp_distance(r[rows, 3:], glibc[rows, 3:]) <= 1).all()
    n_l, n_valid, n_p, und = cand_ref.check_sampled(lat, r, cand_cases.SAMPLE_LATTICE,
                                                    cand_cases.SAMPLE_POSES)
    # (the box covers a quarter of the lattice)
    assert und == 0 and 0.7 * n_l < n_valid < 0.8 * n_l and n_p == rows.size
    ground = r[:, 2] - c["sensor_height"]
    assert (ground != 0).mean() > 0.5           # the terrain is under most of the lattice


@pytest.mark.parametrize("mut", cand_ref.MUTATIONS)
def test_mutation_is_caught(mut):
    name = CAUGHT_BY[mut]
    good, _, _ = _ref(name)
    bad, _, _ = _ref(name, mut)
    assert good.shape != bad.shape or good.tobytes() != bad.tobytes(), \
        f"{mut}: {name} does not tell it from the reference"


def test_every_mutation_has_a_case():
    assert set(CAUGHT_BY) == set(cand_ref.MUTATIONS)
    assert set(CAUGHT_BY.values()) <= set(cand_cases.small_cases())


def _reason_at(name, x, y):
    c = cand_cases.cases()[name]
    xs, ys = cand_cases.lattice_xy(c)
    i, j = int(np.nonzero(xs == x)[0][0]), int(np.nonzero(ys == y)[0][0])
    return _ref(name)[1][i * xs.size + j]


def test_rejections_are_hit_and_on_their_boundaries():
    seen = set()
    for name in cand_cases.small_cases():
        seen |= set(_ref(name)[1])
    assert seen == set(cand_ref.REASONS)
    # zx120: exactly 0.5 away is kept (strict), 0.25 away is dropped
    assert _reason_at("dyadic9", -2.0, -2.0) == "valid" and _reason_at("dyadic9", -1.0, -2.0) == "valid"
    assert _reason_at("dyadic9_zx25", -2.0, -2.0) == "zx"
    assert _ref("dyadic9_zx25")[1].count("zx") == 1 and "zx" not in _ref("dyadic9")[1]
    # the box: its faces and corners are inside (inclusive), one step out is not
    for x, y in ((0.0, 0.0), (4.0, 2.0), (2.0, 4.0), (4.0, 4.0), (0.0, 3.0)):
        assert _reason_at("dyadic9", x, y) == "inside"
    assert _reason_at("dyadic9", -1.0, 0.0) == "valid" and _reason_at("dyadic9", 5.0, 4.0) == "valid"
    assert _ref("dyadic9")[1].count("inside") == 25
    # hd < 0.1: the centre of an inverted box, which nothing is "inside" of
    r = _ref("inverted")[1]
    assert r.count("valid") == 24 and r[12] == "hd" and "inside" not in r
    # the elevation limit: both sides
    for name in ("steep", "steep_sparse"):
        r = _ref(name)[1]
        assert r.count("elev") >= 8 and r.count("valid") >= 8 and r.count("inside") == 1
    # a NaN lattice (gs 1), no lattice (0 candidates), four corners (gs 2)
    assert _ref("gs1")[1] == ["elev"] and _ref("nc0")[1] == [] and _ref("gs2")[1] == ["valid"] * 4
    # radius 0: every lattice point on or inside the box
    assert set(_ref("gs65_r0")[1]) == {"inside"} and len(_ref("gs65_r0")[1]) == 4225
    # the border rings
    assert _ref("gs33")[1].count("valid") == 4 * 32 and _ref("gs65")[1].count("valid") == 4 * 64


def test_axis_angles_are_the_special_values():
    """dyadic9: dz == 0 with no terrain, so every pitch is exactly -pi / 2 (elevation -0.0); the
    8 lattice points on the centre's axes have yaws 0, pi and +-pi / 2 exactly."""
    poses, _, _ = _ref("dyadic9")
    assert (poses[:, 3] == -math.pi / 2).all() and (poses[:, 2] == 1.0).all()
    axis = (poses[:, 0] == 2.0) | (poses[:, 1] == 2.0)
    assert axis.sum() == 8
    assert sorted(set(poses[axis, 4].tolist())) == [-math.pi / 2, 0.0, math.pi / 2, math.pi]
    # an odd lattice over a box symmetric in y: -0.0 and -pi do not occur (dy = cy - y = +0.0)
    assert not np.signbit(poses[axis & (poses[:, 1] == 2.0), 4]).any()


def test_constructed_grounds():
    """The crafted terrains decide what they were built to decide (z - sensor height)."""
    def ground(name, x, y):
        poses = _ref(name)[0]
        k = np.nonzero((poses[:, 0] == x) & (poses[:, 1] == y))[0]
        assert k.size == 1
        return float(poses[k[0], 2]) - cand_cases.cases()[name]["sensor_height"]
    b = "dyadic9_boundaries"
    s3 = float(cand_cases.cases()[b]["terrain"][3, 2])
    assert ground(b, -2.0, -2.0) == 0.0           # 2-D distance exactly 1.0
    assert ground(b, -2.0, 2.0) == 0.0 and ground(b, -2.0, 6.0) == 0.0   # squared distance 4.0f
    assert ground(b, 0.0, -2.0) == s3 and s3 * s3 < 3.0                  # sqrt 3 rounded down
    assert ground(b, 0.0, 6.0) == 0.0                                    # ... and up
    assert ground(b, -2.0, 0.0) == 0.25 and ground(b, 6.0, 0.0) == 0.0   # a float either side of 1
    x0, y0 = cand_cases._fuse_corner()
    assert abs(ground("fuse", x0, y0)) < 1e-15 and abs(ground("fuse", -x0, y0) - 0.7) < 1e-7
    # the straddles: at least 16 lattice points, ground 0.5 (the nearer point in, the farther out)
    c = cand_cases.cases()["nd10_boundaries"]
    pts, dists = cand_cases._nd_boundaries(cand_cases.ND10, 0xB0)
    assert np.array_equal(pts, c["terrain"]) and len(dists) >= 16
    print("nd10 straddles: farthest below 1.0 by %.3g, nearest at or above by %.3g" %
          (max(1.0 - lo for lo, _ in dists), max(hi - 1.0 for _, hi in dists)))
    assert all(1.0 - lo < 1e-9 and hi - 1.0 < 1e-9 for lo, hi in dists)
    for x, y in cand_cases._spread(c):
        assert abs(ground("nd10_boundaries", x, y) - 0.5) < 1e-7
    # sunk: negative wherever there is ground; above / away: none anywhere
    for box in ("dyadic9", "nd10"):
        p = _ref(box + "_sunk")[0]
        h = cand_cases.cases()[box + "_sunk"]["sensor_height"]
        assert (p[:, 2] - h < 0).all()
        for kind in ("above", "away"):
            p = _ref(f"{box}_{kind}")[0]
            assert (p[:, 2] == h).all()
        assert (_ref(box + "_one")[0][:, 2] != h).sum() >= 1
