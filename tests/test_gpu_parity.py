"""GPU parity: libpcp (HIP, gfx950) against the CPU restatement (oracle/) on the same inputs.

Bar (BASELINE.json north_star): crop indices, voxel keys/counts, ray first-hit indices, cell
flags/covered counts and best-pose indices bit-exact; voxel centroids <= 1e-5 m; transformed
xyz exact (same float evaluation order); per-pose score totals (double, correctly rounded acos /
sin against glibc's) bit-identical on the 91-candidate tick, the C5 frames and the long-range
scene (parity.assert_totals_exact), elsewhere within 2 ulps each and at most max(2, 5 %) of them
not bit-identical (parity.assert_totals); per-cell scores at most max(5, 0.4 %) of the positive
ones off, by at most 8 ulps (parity.cell_bar); candidate pitch/yaw (correctly rounded atan2) at
most 2 values one ulp off (tests/parity.py).
All calls go through the C ABI (pointcloud_processor_amd/_abi.py -> libpcp.so).
"""
import ctypes
import math
from pathlib import Path

import numpy as np
import parity
import pytest

from pointcloud_processor_amd import _abi, synth

pytestmark = pytest.mark.gpu

BOX = np.array([0.0, 15.0, -10.0, 10.0, -1.5, 10.0])   # pointcloud_filter.cpp:30-36,111-113
GOLD = Path(__file__).resolve().parent / "golden"
C_u64, C_ref = ctypes.c_uint64, ctypes.byref


def _cloud(n, seed, step_floats=4, nan_frac=0.01):
    rng = np.random.default_rng(seed)
    a = np.zeros((n, step_floats), np.float32)
    a[:, 0] = rng.uniform(-5, 20, n)
    a[:, 1] = rng.uniform(-12, 12, n)
    a[:, 2] = rng.uniform(-3, 12, n)
    if n:
        k = max(1, int(n * nan_frac))
        a[rng.integers(0, n, k), rng.integers(0, 3, k)] = np.nan
        # exact boundary values of the strict box
        b = rng.integers(0, n, min(n, 64))
        a[b[:16], 0] = 0.0
        a[b[16:32], 0] = 15.0
        a[b[32:48], 1] = -10.0
        a[b[48:], 2] = -1.5
    return a


# ---------------------------------------------------------------------------------- filter
@pytest.mark.parametrize("n", [0, 1, 97, 4096, 100_003, 1_000_000])
def test_crop_indices_bit_exact(gpu, oracle, n):
    a = _cloud(n, 1 + n)
    kept, xyz = gpu.crop_box(a, BOX)
    ref = oracle.crop_box(a, BOX)
    np.testing.assert_array_equal(kept, ref)
    np.testing.assert_array_equal(xyz[:, :3], a[ref, :3])


def test_crop_point_step_32_offsets(gpu, oracle):
    a = _cloud(50_000, 7, step_floats=8)
    # fields at x@16, y@20, z@24 of a 32-byte record
    b = np.zeros_like(a)
    b[:, 4:7] = a[:, :3]
    kept, _ = gpu.crop_box(b, BOX, point_step=32, offs=(16, 20, 24))
    np.testing.assert_array_equal(kept, oracle.crop_box(a, BOX))


@pytest.mark.parametrize("n,leaf", [(1, 0.2), (5000, 0.2), (300_000, 0.2), (300_000, 0.05),
                                    (2_000_000, 0.05)])
def test_voxel_grid_exact(gpu, oracle, n, leaf):
    a = _cloud(n, 11 + n, nan_frac=0.0)
    out, idx, cnt, pt = gpu.voxel_grid(a, leaf)
    r_xyz, r_idx, r_cnt, r_pt = oracle.voxel_grid(a, leaf)
    assert pt == r_pt
    np.testing.assert_array_equal(idx, r_idx)
    np.testing.assert_array_equal(cnt, r_cnt)
    # same (stable) in-voxel summation order -> identical floats; the reference's own
    # spreadsort order may differ, hence the documented 1e-5 m tolerance
    np.testing.assert_allclose(out[:, :3], r_xyz, rtol=0, atol=1e-5)
    assert np.array_equal(out[:, :3], r_xyz)


@pytest.mark.parametrize("n,span", [(200_000, 1.0), (100_000, 0.01)])
def test_voxel_grid_dense_voxels(gpu, oracle, n, span):
    """Thousands of points per voxel (span 1 m / leaf 0.2 = 125 voxels) and a single voxel
    holding every point: segments crossing many sort tiles, long in-order centroid sums."""
    rng = np.random.default_rng(n)
    a = np.zeros((n, 4), np.float32)
    a[:, :3] = rng.uniform(0.0, span, (n, 3))
    out, idx, cnt, pt = gpu.voxel_grid(a, 0.2)
    r_xyz, r_idx, r_cnt, _ = oracle.voxel_grid(a, 0.2)
    assert not pt
    np.testing.assert_array_equal(idx, r_idx)
    np.testing.assert_array_equal(cnt, r_cnt)
    np.testing.assert_array_equal(out[:, :3], r_xyz)


def test_voxel_grid_nan_and_overflow(gpu, oracle):
    a = _cloud(20_000, 3, nan_frac=0.05)
    out, idx, cnt, pt = gpu.voxel_grid(a, 0.2)
    fin = np.isfinite(a[:, :3]).all(1)
    r_xyz, r_idx, r_cnt, _ = oracle.voxel_grid(a[fin], 0.2)
    np.testing.assert_array_equal(idx, r_idx)
    np.testing.assert_array_equal(out[:, :3], r_xyz)
    # PCL int32 overflow guard -> passthrough of the (finite) input
    big = np.array([[0, 0, 0, 0], [1000, 1000, 1000, 0], [5, 5, 5, 0]], np.float32)
    out, idx, cnt, pt = gpu.voxel_grid(big, 0.001)
    r_xyz, _, _, r_pt = oracle.voxel_grid(big, 0.001)
    assert pt and r_pt
    np.testing.assert_array_equal(out[:, :3], r_xyz)


@pytest.mark.parametrize("leaf", [0.0, 0.2])
def test_crop_voxel_pipeline(gpu, oracle, leaf):
    a = _cloud(400_000, 5)
    out, ncrop = gpu.crop_voxel(a, BOX, leaf)
    kept = oracle.crop_box(a, BOX)
    assert ncrop == kept.size
    if leaf > 0:
        r_xyz, _, _, _ = oracle.voxel_grid(a[kept], leaf)
    else:
        r_xyz = a[kept, :3]
    np.testing.assert_array_equal(out[:, :3], r_xyz)


@pytest.mark.parametrize("seed", range(8))
def test_crop_voxel_random_boxes(gpu, oracle, seed):
    """Random boxes, leaf sizes and clouds with a third of the coordinates on the 0.05 grid (box
    faces and voxel boundaries), through the GPU crop + voxel against the oracle."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 300_000))
    a = rng.uniform(-6, 6, (n, 4)).astype(np.float32)
    k = n // 3
    a[:k, :3] = (np.round(a[:k, :3] / np.float32(0.05)) * np.float32(0.05)).astype(np.float32)
    lo = rng.uniform(-5, 1, 3)
    box = np.array([lo[0], lo[0] + rng.uniform(0, 8), lo[1], lo[1] + rng.uniform(0, 8),
                    lo[2], lo[2] + rng.uniform(0, 8)])
    box[::2] = np.round(box[::2] / 0.05) * 0.05      # faces on the grid too
    leaf = float(rng.choice([0.0, 0.05, 0.1, 0.2, 0.37]))
    out, ncrop = gpu.crop_voxel(a, box, leaf)
    kept = oracle.crop_box(a, box)
    assert ncrop == kept.size
    ref = oracle.voxel_grid(a[kept], leaf)[0] if leaf > 0 and kept.size else a[kept, :3]
    np.testing.assert_array_equal(out[:, :3], ref)


# ---------------------------------------------------------------------------------- merger
def _tfs():
    yaw = math.radians(30.0)
    q_robot = (0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2))
    return [((8.0, -3.0, 0.0), q_robot), ((0.55, 0.4, 3.5), (0.0, math.sin(0.4363 / 2), 0.0,
                                                              math.cos(0.4363 / 2)))]


def test_transform_concat_exact(gpu, oracle):
    a = _cloud(70_001, 21, nan_frac=0.0)
    b = _cloud(33_333, 22, nan_frac=0.0)
    tfs = _tfs()
    rgbs = [(255, 0, 0), (0, 0, 255)]
    out = gpu.transform_concat([a, b], tfs, rgbs)
    ref = np.concatenate([oracle.transform_rgb(a, *tfs[0], rgbs[0]),
                          oracle.transform_rgb(b, *tfs[1], rgbs[1])])
    assert out.shape == ref.shape
    np.testing.assert_array_equal(out[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))


def test_filter_merge_pipeline(gpu, oracle):
    a = synth.lidar_cloud(300_000, seed=1)
    b = synth.lidar_cloud(200_000, seed=2, sensor_height=3.5)
    tfs = _tfs()
    rgbs = [(255, 0, 0), (0, 0, 255)]
    out, per = gpu.filter_merge([a, b], [BOX, BOX], 0.05, tfs, rgbs)
    parts = []
    for c, tf, rgb in zip([a, b], tfs, rgbs):
        k = oracle.crop_box(c, BOX)
        v, _, _, _ = oracle.voxel_grid(c[k], 0.05)
        parts.append(oracle.transform_rgb(v, *tf, rgb))
    ref = np.concatenate(parts)
    assert list(per) == [p.shape[0] for p in parts]
    np.testing.assert_array_equal(out[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))


def test_filter_merge_full_c3_frame(gpu, oracle):
    """The whole C3 frame of bench.py --mode filter (2 x 5 M LiDAR-like points, crop + voxel
    0.05 + transform + colour): every output record bit-exact against the oracle."""
    import math

    a = synth.lidar_cloud(5_000_000, sensor_height=2.0, seed=1)
    b = synth.lidar_cloud(5_000_000, sensor_height=3.5, seed=2)
    yaw = math.radians(30.0)
    tfs = [((8.0, -3.0, 0.0), (0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2))),
           ((0.55, 0.4, 3.5), (0.0, math.sin(0.4363 / 2), 0.0, math.cos(0.4363 / 2)))]
    rgbs = [(255, 0, 0), (0, 0, 255)]
    out, per = gpu.filter_merge([a, b], [BOX, BOX], 0.05, tfs, rgbs)
    parts = []
    for c, tf, rgb in zip([a, b], tfs, rgbs):
        k = oracle.crop_box(c, BOX)
        v, _, _, _ = oracle.voxel_grid(c[k], 0.05)
        parts.append(oracle.transform_rgb(v, *tf, rgb))
    ref = np.concatenate(parts)
    assert list(per) == [p.shape[0] for p in parts]
    np.testing.assert_array_equal(out[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))


@pytest.mark.parametrize("second", ["direct", "unbounded", "empty"])
def test_filter_merge_sparse_survivors(gpu, oracle, second):
    """A certainly-voxelised cloud whose ~3,000 survivors are spread over ~1,500 crop tiles
    (one sort tile spans more crop tiles than the first sort pass stages in LDS), batched with a
    second cloud that is voxelised the same way, through the compaction-kernel path (unbounded
    box) or is empty; three calls in a row (the crop's block tickets reset)."""
    rng = np.random.default_rng(77)
    n = 6_000_000
    a = rng.uniform(20.0, 40.0, (n, 4)).astype(np.float32)          # outside BOX
    idx = rng.choice(n, 3000, replace=False)
    a[idx, :3] = rng.uniform([0.5, -5.0, 0.0], [10.0, 5.0, 5.0], (3000, 3)).astype(np.float32)
    b = synth.lidar_cloud(150_000, seed=3) if second != "empty" else np.zeros((0, 4), np.float32)
    box_b = BOX if second != "unbounded" else np.array([-np.inf, np.inf] * 3)
    tfs = _tfs()
    rgbs = [(255, 0, 0), (0, 0, 255)]
    parts = []
    for c, box, tf, rgb in zip([a, b], [BOX, box_b], tfs, rgbs):
        if c.shape[0] == 0:
            continue
        k = oracle.crop_box(c, box)
        v, _, _, pt = oracle.voxel_grid(c[k], 0.05)
        assert not pt
        parts.append(oracle.transform_rgb(v, *tf, rgb))
    ref = np.concatenate(parts)
    for _ in range(3):
        out, per = gpu.filter_merge([a, b], [BOX, box_b], 0.05, tfs, rgbs)
        assert list(per)[:len(parts)] == [p.shape[0] for p in parts]
        np.testing.assert_array_equal(out[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))


@pytest.mark.parametrize("case", ["dense_groups", "far_box", "one_pass", "fine_leaf"])
def test_filter_merge_fast_chain(gpu, oracle, case, monkeypatch):
    """The fast chain (box-relative keys formed in the crop, pass 0 straight from the crop
    tiles in groups of 8) against the oracle and the general chain (PCP_FM_FAST=0):
    dense_groups -- every point survives, so one pass-0 group holds 8 x 4096 items (8 chunks)
    and one voxel holds 100 k points; far_box -- a box 2 km from the origin with negative
    coordinates; one_pass -- a box of < 2^9 voxels (a single radix pass); fine_leaf -- leaf
    0.013 m (four passes over the key)."""
    rng = np.random.default_rng({"dense_groups": 1, "far_box": 2, "one_pass": 3,
                                 "fine_leaf": 4}[case])
    leaf = 0.05
    if case == "dense_groups":
        box = np.array([-1.0, 30.0, -10.0, 10.0, -3.0, 5.0])
        a = np.zeros((200_000, 4), np.float32)
        a[:, :3] = rng.uniform([0, -5, -1], [20, 5, 2], (200_000, 3))
        a[50_000:150_000, :3] = [3.01, 2.02, 0.33]
        b = synth.lidar_cloud(100_000, seed=8)
    elif case == "far_box":
        box = np.array([-2105.0, -2085.0, 1990.0, 2010.0, -1.5, 9.0])
        a = np.zeros((400_000, 4), np.float32)
        a[:, :3] = rng.uniform([-2110, 1985, -3], [-2080, 2015, 10], (400_000, 3))
        b = a[::-1].copy()
    elif case == "one_pass":
        box = np.array([1.0, 1.3, -0.2, 0.1, 0.0, 0.2])
        a = np.zeros((300_000, 4), np.float32)
        a[:, :3] = rng.uniform([0.8, -0.4, -0.1], [1.5, 0.3, 0.3], (300_000, 3))
        b = a.copy()
        b[:, 2] += np.float32(0.05)
    else:
        leaf = 0.013
        box = np.array([0.0, 15.0, -10.0, 10.0, -1.5, 1.5])
        a = synth.lidar_cloud(600_000, seed=9)
        b = synth.lidar_cloud(400_000, seed=10, sensor_height=3.5)
    tfs = _tfs()
    rgbs = [(255, 0, 0), (0, 0, 255)]
    parts = []
    for c, tf, rgb in zip([a, b], tfs, rgbs):
        k = oracle.crop_box(c, box)
        v, _, _, pt = oracle.voxel_grid(c[k], leaf)
        assert not pt
        parts.append(oracle.transform_rgb(v, *tf, rgb))
    ref = np.concatenate(parts)
    out, per = gpu.filter_merge([a, b], [box, box], leaf, tfs, rgbs)
    assert list(per) == [p.shape[0] for p in parts]
    np.testing.assert_array_equal(out[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))
    monkeypatch.setenv("PCP_FM_FAST", "0")
    ctx = _abi.Context(0)
    try:
        out2, per2 = ctx.filter_merge([a, b], [box, box], leaf, tfs, rgbs)
    finally:
        ctx.close()
    assert list(per2) == list(per)
    np.testing.assert_array_equal(out2.view(np.uint32), out.view(np.uint32))


@pytest.mark.parametrize("case", ["lidar", "three_clouds", "tiny", "one_bucket", "dense_redo",
                                  "near_cap", "dense_voxel"])
def test_filter_merge_bucket_chain(oracle, case, monkeypatch):
    """The bucket chain (PCP_FM_FAST=2, the default: crop -> per-group counting sort by bucket ->
    per-bucket LDS sort + input-order sums + look-back offsets) against the oracle and the LSD
    fast chain (PCP_FM_FAST=1).  lidar: two LiDAR clouds; three_clouds: a middle cloud with
    nothing cropped (no buckets) between two that voxelise; tiny: 5 points; one_bucket: a box of
    < 2^11 voxels (one bucket, bs = 0); dense_redo: one voxel of 60 k points (its bucket passes
    the LDS capacity, the frame is redone on the LSD chain: voxel_redo counts it); near_cap: a
    dense cluster whose bucket stays just under the capacity, but whose ONE voxel of ~3,500
    points passes kBkDense (512: the in-voxel rank is quadratic) -- redone too;
    dense_voxel: 400 points in one voxel, ranked in the bucket chain."""
    rng = np.random.default_rng(50 + len(case))
    tfs = _tfs()
    rgbs = [(255, 0, 0), (0, 0, 255)]
    box = BOX
    redo = 0
    if case == "lidar":
        clouds = [synth.lidar_cloud(700_000, seed=31), synth.lidar_cloud(500_000, seed=32,
                                                                         sensor_height=3.5)]
    elif case == "three_clouds":
        far = rng.uniform(30, 40, (50_000, 4)).astype(np.float32)
        clouds = [synth.lidar_cloud(200_000, seed=33), far, synth.lidar_cloud(90_000, seed=34)]
        tfs = [tfs[0], tfs[1], tfs[0]]
        rgbs = [(255, 0, 0), (0, 255, 0), (0, 0, 255)]
    elif case == "tiny":
        clouds = [np.array([[1, 1, 1, 0], [1.01, 1.01, 1.01, 0], [5, -3, 2, 0], [2, 2, 2, 0],
                            [1.02, 1.0, 1.03, 0]], np.float32), synth.lidar_cloud(1000, seed=35)]
    elif case == "one_bucket":
        box = np.array([1.0, 1.5, -0.2, 0.3, 0.0, 0.2])
        a = np.zeros((200_000, 4), np.float32)
        a[:, :3] = rng.uniform([0.9, -0.3, -0.1], [1.6, 0.4, 0.3], (200_000, 3))
        clouds = [a, a[::-1].copy()]
    elif case == "dense_redo":
        a = synth.lidar_cloud(300_000, seed=36)
        a[100_000:160_000, :3] = [3.01, 2.02, 0.33]
        clouds = [a, synth.lidar_cloud(100_000, seed=37)]
        redo = 1
    elif case == "near_cap":   # ~3,500 points in one voxel of an otherwise sparse cloud
        a = synth.lidar_cloud(200_000, seed=38)
        a[50_000:53_500, :3] = [7.51, -1.02, 0.43]
        clouds = [a, synth.lidar_cloud(100_000, seed=39)]
        redo = 1
    else:   # dense_voxel: 400 points in one voxel (under kBkDense), spread over the input
        a = synth.lidar_cloud(200_000, seed=40)
        a[7:200_000:500, :3] = [4.26, 3.17, 0.12]
        clouds = [a, synth.lidar_cloud(100_000, seed=41)]
    parts = []
    for c, tf, rgb in zip(clouds, tfs, rgbs):
        k = oracle.crop_box(c, box)
        if k.size == 0:
            parts.append(np.zeros((0, 8), np.float32))
            continue
        v, _, _, pt = oracle.voxel_grid(c[k], 0.05)
        assert not pt
        parts.append(oracle.transform_rgb(v, *tf, rgb))
    ref = np.concatenate(parts)
    outs = {}
    for mode in ("2", "1"):
        monkeypatch.setenv("PCP_FM_FAST", mode)
        ctx = _abi.Context(0)
        try:
            for _ in range(2):
                out, per = ctx.filter_merge(clouds, [box] * len(clouds), 0.05, tfs, rgbs)
                assert list(per) == [p.shape[0] for p in parts]
                np.testing.assert_array_equal(out[:, :5].view(np.uint32),
                                              ref[:, :5].view(np.uint32))
            outs[mode] = out
            if mode == "2":
                assert ctx.profile_get("voxel_redo")[1] == 2 * redo
        finally:
            ctx.close()
    np.testing.assert_array_equal(outs["2"].view(np.uint32), outs["1"].view(np.uint32))


@pytest.mark.parametrize("case", ["scans", "dense_redo", "empty_crop"])
def test_filter_merge_nodes(gpu, oracle, case):
    """pcp_filter_merge_nodes (the filter node for both sensors + the merger node composed, ONE
    synchronisation): each cloud's filtered message bit-identical to pcp_crop_voxel's (and the
    oracle's crop + VoxelGrid), the merged records bit-identical to pcp_transform_concat over
    them (and the oracle's), the cropped counts exact.  scans: two C5 scans (leaf 0.2, bucket
    chain); dense_redo: a 60 k-point voxel (the bucket chain's redo -> the general chain);
    empty_crop: a cloud with nothing in its box."""
    rng = np.random.default_rng(77)
    a = synth.lidar_cloud(60_032, sensor_height=2.0, seed=101)
    b = synth.lidar_cloud(60_032, sensor_height=3.5, seed=102)
    leaf = 0.2
    if case == "dense_redo":
        a = synth.lidar_cloud(200_000, seed=36)
        a[10_000:70_000, :3] = [3.01, 2.02, 0.33]
        leaf = 0.05
    elif case == "empty_crop":
        b = rng.uniform(30, 40, (5_000, 4)).astype(np.float32)
    clouds = [a, b]
    tfs = [((8.0, -3.0, 2.0), (0.0, 0.0, 0.2588190451025208, 0.9659258262890683)),
           ((0.55, 0.4, 3.5), (0.0, 0.21633, 0.0, 0.97632))]
    rgbs = [(255, 0, 0), (0, 0, 255)]
    merged, filt, crop = gpu.filter_merge_nodes(clouds, [BOX, BOX], leaf, tfs, rgbs)
    # the same bytes where they landed (pcp_filter_merge_landed: what the C++ composed front
    # builds its messages from and the composed carve reads in place)
    mp = ctypes.c_void_p()
    fp = (ctypes.c_void_p * 2)()
    assert gpu.lib.pcp_filter_merge_landed(gpu.h, 2, ctypes.byref(mp), fp) == 0
    if merged.size:
        got = np.ctypeslib.as_array(ctypes.cast(mp, ctypes.POINTER(ctypes.c_float)),
                                    (merged.shape[0], 8))
        np.testing.assert_array_equal(got.view(np.uint32), merged.view(np.uint32))
    for i, f in enumerate(filt):
        if f.shape[0]:
            got = np.ctypeslib.as_array(ctypes.cast(fp[i], ctypes.POINTER(ctypes.c_float)),
                                        (f.shape[0], 4))
            np.testing.assert_array_equal(got[:, :3].view(np.uint32), f[:, :3].view(np.uint32))
    assert gpu.lib.pcp_filter_merge_landed(gpu.h, 3, ctypes.byref(mp), fp) != 0   # (k differs)
    ref_f = []
    for c, f, m in zip(clouds, filt, crop):
        kept = oracle.crop_box(c, BOX)
        assert int(m) == kept.size
        v = oracle.voxel_grid(c[kept], leaf)[0] if kept.size else np.zeros((0, 3), np.float32)
        np.testing.assert_array_equal(f[:, :3], v)
        g, ncrop = gpu.crop_voxel(c, BOX, leaf)
        assert ncrop == kept.size
        np.testing.assert_array_equal(f[:, :3], g[:, :3])
        ref_f.append(v)
    ref = np.concatenate([oracle.transform_rgb(v, *tf, rgb) for v, tf, rgb in
                          zip(ref_f, tfs, rgbs)])
    np.testing.assert_array_equal(merged[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))
    tc = gpu.transform_concat([f[:, :3].copy() for f in filt], tfs, rgbs)
    np.testing.assert_array_equal(merged[:, :5].view(np.uint32), tc[:, :5].view(np.uint32))


def test_crop_voxel_bucket_chain_voxel_order(gpu, oracle):
    """pcp_voxel_grid's idx / count outputs come from the general chain; pcp_crop_voxel's
    centroids from the bucket chain (run_single): the same centroids, in PCL idx order."""
    a = synth.lidar_cloud(400_000, seed=41)
    out, ncrop = gpu.crop_voxel(a, BOX, 0.05)
    kept = oracle.crop_box(a, BOX)
    r_xyz, r_idx, r_cnt, _ = oracle.voxel_grid(a[kept], 0.05)
    assert ncrop == kept.size
    np.testing.assert_array_equal(out[:, :3], r_xyz)
    assert np.all(np.diff(r_idx.astype(np.int64)) > 0)


def test_filter_merge_device_graph_replay(gpu, oracle):
    """Device-resident inputs: the pipeline is captured into a hipGraph and replayed; every
    replay must equal the eager host-path result and the oracle."""
    a = synth.lidar_cloud(250_000, seed=5)
    b = synth.lidar_cloud(150_000, seed=6, sensor_height=3.5)
    tfs = _tfs()
    rgbs = [(255, 0, 0), (0, 0, 255)]
    ref, per_ref = gpu.filter_merge([a, b], [BOX, BOX], 0.05, tfs, rgbs)
    dp = [gpu.dev_alloc(c.nbytes) for c in (a, b)]
    for p, c in zip(dp, (a, b)):
        gpu.h2d(p, c)
    views = [_abi.CloudView(p, c.shape[0], 16, 0, 4, 8) for p, c in zip(dp, (a, b))]
    cap = a.shape[0] + b.shape[0]
    out_d = gpu.dev_alloc(cap * 32)
    try:
        for _ in range(3):   # capture, then replays
            n, per = gpu.filter_merge_device(views, [BOX, BOX], 0.05, tfs, rgbs, out_d, cap)
            assert n == ref.shape[0] and list(per) == list(per_ref)
            got = np.empty((n, 8), np.float32)
            gpu.d2h(got, out_d)
            np.testing.assert_array_equal(got[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))
        # the prepared steady-state call replays the same graph
        frame = gpu.filter_merge_device_prepared(views, [BOX, BOX], 0.05, tfs, rgbs, out_d, cap)
        for _ in range(2):
            n3, per3 = frame()
            assert n3 == ref.shape[0] and list(per3) == list(per_ref)
            got = np.empty((n3, 8), np.float32)
            gpu.d2h(got, out_d)
            np.testing.assert_array_equal(got[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))
        # a different box invalidates the captured graph
        box2 = BOX.copy()
        box2[1] = 8.0
        n2, _ = gpu.filter_merge_device(views, [box2, box2], 0.05, tfs, rgbs, out_d, cap)
        ref2, _ = gpu.filter_merge([a, b], [box2, box2], 0.05, tfs, rgbs)
        assert n2 == ref2.shape[0] and n2 < n
    finally:
        for p in dp + [out_d]:
            gpu.dev_free(p)
    parts = []
    for c, tf, rgb in zip([a, b], tfs, rgbs):
        k = oracle.crop_box(c, BOX)
        v, _, _, _ = oracle.voxel_grid(c[k], 0.05)
        parts.append(oracle.transform_rgb(v, *tf, rgb))
    np.testing.assert_array_equal(ref[:, :5].view(np.uint32),
                                  np.concatenate(parts)[:, :5].view(np.uint32))


def test_filter_merge_device_graph_redo(oracle):
    """Device-resident inputs through the captured graph when the bucket chain must redo the
    frame (one 30 k-point voxel: its bucket passes the LDS capacity): every replay redoes the
    frame on the LSD chain inside the call and returns the oracle's bytes; a later frame whose
    buckets fit replays the same graph without a redo."""
    a = synth.lidar_cloud(200_000, seed=61)
    a[20_000:50_000, :3] = [4.01, -2.02, 0.51]
    b = synth.lidar_cloud(100_000, seed=62, sensor_height=3.5)
    tfs = _tfs()
    rgbs = [(255, 0, 0), (0, 0, 255)]
    parts = []
    for c, tf, rgb in zip([a, b], tfs, rgbs):
        k = oracle.crop_box(c, BOX)
        v, _, _, _ = oracle.voxel_grid(c[k], 0.05)
        parts.append(oracle.transform_rgb(v, *tf, rgb))
    ref = np.concatenate(parts)
    ctx = _abi.Context(0)
    dp = [ctx.dev_alloc(c.nbytes) for c in (a, b)]
    cap = a.shape[0] + b.shape[0]
    out_d = ctx.dev_alloc(cap * 32)
    try:
        for p, c in zip(dp, (a, b)):
            ctx.h2d(p, c)
        views = [_abi.CloudView(p, c.shape[0], 16, 0, 4, 8) for p, c in zip(dp, (a, b))]
        for i in range(3):   # capture, then replays
            n, per = ctx.filter_merge_device(views, [BOX, BOX], 0.05, tfs, rgbs, out_d, cap)
            assert n == ref.shape[0] and list(per) == [p.shape[0] for p in parts]
            got = np.empty((n, 8), np.float32)
            ctx.d2h(got, out_d)
            np.testing.assert_array_equal(got[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))
            assert ctx.profile_get("voxel_redo")[1] == i + 1
        # the dense voxel gone (same views, same graph): no redo
        a2 = synth.lidar_cloud(200_000, seed=61)
        ctx.h2d(dp[0], a2)
        n2, _ = ctx.filter_merge_device(views, [BOX, BOX], 0.05, tfs, rgbs, out_d, cap)
        assert ctx.profile_get("voxel_redo")[1] == 3
        k2 = oracle.crop_box(a2, BOX)
        v2, _, _, _ = oracle.voxel_grid(a2[k2], 0.05)
        ref2 = np.concatenate([oracle.transform_rgb(v2, *tfs[0], rgbs[0]), parts[1]])
        got = np.empty((n2, 8), np.float32)
        ctx.d2h(got, out_d)
        np.testing.assert_array_equal(got[:, :5].view(np.uint32), ref2[:, :5].view(np.uint32))
    finally:
        for p in dp + [out_d]:
            ctx.dev_free(p)
        ctx.close()


def test_filter_merge_pinned_staging(gpu):
    """PointCloud2 boundary with page-locked buffers: clouds and the output pinned in place
    (pcp_host_register) and a pcp_host_alloc block must give the pageable path's bytes."""
    a = synth.lidar_cloud(120_000, seed=9)
    b = synth.lidar_cloud(80_000, seed=10, sensor_height=3.5)
    tfs = _tfs()
    rgbs = [(255, 0, 0), (0, 0, 255)]
    ref, per_ref = gpu.filter_merge([a, b], [BOX, BOX], 0.05, tfs, rgbs)
    out = np.empty((a.shape[0] + b.shape[0], 8), np.float32)
    for x in (a, b, out):
        gpu.host_register(x)
    try:
        got, per = gpu.filter_merge([a, b], [BOX, BOX], 0.05, tfs, rgbs, out=out)
        assert list(per) == list(per_ref)
        np.testing.assert_array_equal(got[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))
    finally:
        for x in (a, b, out):
            gpu.host_unregister(x)
    # a pinned allocation from the library, filled in place and used as the input cloud
    hp = ctypes.c_void_p()
    assert gpu.lib.pcp_host_alloc(gpu.h, a.nbytes, C_ref(hp)) == 0 and hp.value
    try:
        pinned = np.ctypeslib.as_array(ctypes.cast(hp, ctypes.POINTER(ctypes.c_float)),
                                       shape=a.shape)
        pinned[:] = a
        got, per = gpu.filter_merge([pinned, b], [BOX, BOX], 0.05, tfs, rgbs)
        assert list(per) == list(per_ref)
        np.testing.assert_array_equal(got[:, :5].view(np.uint32), ref[:, :5].view(np.uint32))
    finally:
        assert gpu.lib.pcp_host_free(gpu.h, hp) == 0
    with pytest.raises(ValueError):                       # output too small
        gpu.filter_merge([a, b], [BOX, BOX], 0.05, tfs, rgbs, out=out[:10])


# ---------------------------------------------------------------------------------- virtual_lidar
@pytest.fixture(scope="module")
def loaded(gpu, oracle, scene, cells, aux):
    gpu.set_terrain(scene.terrain, point_step=32)
    gpu.set_aux_cloud(aux, point_step=32)
    gpu.set_cells(cells.xyz, cells.normals)
    T = oracle.Cloud(scene.terrain)
    A = oracle.Cloud(aux)
    return T, A


def test_terrain_index_info(gpu, loaded, scene):
    info = gpu.terrain_info()
    assert info["n_points"] == scene.terrain.shape[0]
    assert info["cell"] >= 2 * (0.08 * 0.7)


def test_candidates_match(gpu, oracle, loaded, scene, cells):
    """generateCandidatePositions: positions bit-exact; pitch and yaw (atan2, correctly rounded
    on the device, pcp_crmath.h) bit-identical to glibc's but for its rare near-tie misroundings
    (at most 2 values here, one ulp each: tests/parity.py; ocml's own atan2 left ~8 % one ulp
    off)."""
    T, _ = loaded
    for nc in (100, 400, 1000):
        p = _abi.default_vl_params(num_candidates=nc)
        g = gpu.generate_candidates(cells.grid_bbox, p, scene.zx120_pose5)
        r = oracle.generate_candidates(T, cells.grid_bbox, oracle.vl_params(num_candidates=nc),
                                       scene.zx120_pose5)
        assert g.shape == r.shape
        np.testing.assert_array_equal(g[:, :3], r[:, :3])
        np.testing.assert_allclose(g[:, 3:], r[:, 3:], rtol=0, atol=1e-12)
        parity.assert_angles(g[:, 3:], r[:, 3:])   # <= 2 values, one ulp each


def test_step_table():
    s = _abi.step_table(15.0 - 0.08)
    assert s.size == 49 and s[0] == 0.5
    ref = [0.5]
    while True:
        x = ref[-1] + 0.3
        if not x < 15.0 - 0.08:
            break
        ref.append(x)
    assert np.array_equal(s, np.array(ref))


def test_raycast_fan_first_hit_exact(gpu, oracle, loaded, scene, cells):
    T, _ = loaded
    p = _abi.default_vl_params(num_candidates=100)
    poses = gpu.generate_candidates(cells.grid_bbox, p, scene.zx120_pose5)[:6]
    fan = _abi.fan_params(n_az=256, n_el=64)
    blocked, units, fh, best = gpu.raycast_fan(poses, fan, want_first_hit=True)
    r_blocked, r_units, r_fh = oracle.raycast_fan(T, poses, 256, 64, fan.el_min, fan.el_max,
                                                  fan.max_distance)
    np.testing.assert_array_equal(fh, r_fh)
    np.testing.assert_array_equal(blocked, r_blocked)
    np.testing.assert_array_equal(units, r_units)
    assert best == int(np.argmin(r_blocked))
    # depths = step table entries (exact), within the 1e-4 m bar trivially
    steps = _abi.step_table(fan.max_distance - 0.08)
    d = np.where(fh >= 0, steps[np.maximum(fh, 0)], np.nan)
    rd = np.where(r_fh >= 0, steps[np.maximum(r_fh, 0)], np.nan)
    np.testing.assert_allclose(d, rd, atol=1e-4, equal_nan=True)


def test_raycast_fan_random_poses(gpu, oracle, loaded, scene):
    """Poses anywhere around the terrain: inside and outside its bbox, below the ground, in
    the pit, at any pitch/yaw; odd fan sizes and elevation limits."""
    T, _ = loaded
    rng = np.random.default_rng(7)
    pts = scene.terrain[:, :3]
    lo, hi = pts.min(0) - 3.0, pts.max(0) + 3.0
    poses = np.column_stack([rng.uniform(lo[0], hi[0], 24), rng.uniform(lo[1], hi[1], 24),
                             rng.uniform(lo[2] - 1.0, hi[2] + 3.0, 24),
                             rng.uniform(-1.5, 1.5, 24), rng.uniform(-np.pi, np.pi, 24)])
    for n_az, n_el, el_lo, el_hi, dmax in ((96, 17, -80.0, 80.0, 15.0), (130, 9, -17.0, 6.0, 7.5)):
        fan = _abi.fan_params(n_az=n_az, n_el=n_el, el_min_deg=el_lo, el_max_deg=el_hi,
                              max_distance=dmax)
        blocked, units, fh, _ = gpu.raycast_fan(poses, fan, want_first_hit=True)
        r_blocked, r_units, r_fh = oracle.raycast_fan(T, poses, n_az, n_el, fan.el_min,
                                                      fan.el_max, dmax)
        np.testing.assert_array_equal(fh, r_fh)
        np.testing.assert_array_equal(blocked, r_blocked)
        np.testing.assert_array_equal(units, r_units)


def test_into_wrappers_match(gpu, loaded, scene, cells):
    """The allocation-free steady-state calls give the allocating calls' results."""
    p = _abi.default_vl_params(num_candidates=100)
    poses = np.ascontiguousarray(gpu.generate_candidates(cells.grid_bbox, p, scene.zx120_pose5))
    fan = _abi.fan_params(n_az=128, n_el=16)
    blocked, units, _, best = gpu.raycast_fan(poses, fan)
    b2 = np.zeros(poses.shape[0], np.uint32)
    u2 = np.zeros(poses.shape[0], np.uint64)
    assert gpu.raycast_fan_into(poses, fan, b2, u2) == best
    np.testing.assert_array_equal(b2, blocked)
    np.testing.assert_array_equal(u2, units)
    f1 = np.zeros(cells.xyz.shape[0], np.uint8)
    f2 = f1.copy()
    tot, cov, rep = gpu.score_poses(poses, scene.zx120_pose5, p, f1)
    t2 = np.zeros(poses.shape[0], np.float64)
    c2 = np.zeros(poses.shape[0], np.int32)
    r2 = _abi.VlReport()
    gpu.score_poses_into(poses, np.ascontiguousarray(scene.zx120_pose5, np.float64), p, f2, t2, c2,
                         r2)
    np.testing.assert_array_equal(t2, tot)
    np.testing.assert_array_equal(c2, cov)
    np.testing.assert_array_equal(f2, f1)
    assert r2.best_idx == rep.best_idx and r2.green == rep.green


@pytest.mark.parametrize("npw,tile,skip", [("1", "2", "1"), ("2", "2", "1"), ("8", "2", "1"),
                                           ("8", "1", "1"), ("8", "2", "2")])
def test_raycast_fan_poses_per_wave(oracle, loaded, scene, cells, npw, tile, skip, monkeypatch):
    """64 poses (P % 64 == 0: the XCD-chunk kernel with NPW poses per wave, its step table in
    LDS) on split and 8-byte fine records, split records with one or two walk-start skip
    thresholds (PCP_FINE_SKIP): blocked counts, units and first hits exact."""
    T, _ = loaded
    monkeypatch.setenv("PCP_FAN_NPW", npw)
    monkeypatch.setenv("PCP_FINE_SKIP", skip)
    monkeypatch.setenv("PCP_FINE_TILE", tile.rstrip("u"))
    monkeypatch.setenv("PCP_FINE_PACK", "0" if tile.endswith("u") else "1")
    monkeypatch.setenv("PCP_TERRAIN_BLOCKS", "2")
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(scene.terrain, point_step=32)
        p = _abi.default_vl_params(num_candidates=100)
        poses = ctx.generate_candidates(cells.grid_bbox, p, scene.zx120_pose5)
        poses = np.ascontiguousarray(np.resize(poses, (64, 5)))
        fan = _abi.fan_params(n_az=256, n_el=32)
        blocked, units, fh, best = ctx.raycast_fan(poses, fan, want_first_hit=True)
        info = ctx.terrain_info()
        assert info["scan_layout"] == "fine" and info["fine_tile"] == int(tile)
    finally:
        ctx.close()
    oracle.set_threads(8)
    r_blocked, r_units, r_fh = oracle.raycast_fan(T, poses, 256, 32, fan.el_min, fan.el_max,
                                                  fan.max_distance)
    oracle.set_threads(1)
    np.testing.assert_array_equal(fh, r_fh)
    np.testing.assert_array_equal(blocked, r_blocked)
    np.testing.assert_array_equal(units, r_units)
    assert best == int(np.argmin(r_blocked))


def test_raycast_fan_full_size_two_poses(gpu, oracle, loaded, scene, cells):
    """BASELINE configs[1] fan (1024 x 256) on two poses, bit-exact against the oracle."""
    T, _ = loaded
    p = _abi.default_vl_params(num_candidates=400)
    poses = gpu.generate_candidates(cells.grid_bbox, p, scene.zx120_pose5)
    poses = poses[[0, len(poses) // 2]]
    fan = _abi.fan_params()
    blocked, units, fh, best = gpu.raycast_fan(poses, fan, want_first_hit=True)
    oracle.set_threads(8)
    r_blocked, r_units, r_fh = oracle.raycast_fan(T, poses, 1024, 256, fan.el_min, fan.el_max,
                                                  fan.max_distance)
    oracle.set_threads(1)
    np.testing.assert_array_equal(fh, r_fh)
    np.testing.assert_array_equal(blocked, r_blocked)
    np.testing.assert_array_equal(units, r_units)


def _clutter_cloud(seed=17):
    """A volumetric cloud (not a surface): a noisy floor, a dense box of random points, a thin
    vertical wall and a few isolated points -- cells hold many points spread in z, so the z
    bands are wide and the run walks go deep."""
    rng = np.random.default_rng(seed)
    floor = np.c_[rng.uniform(-6, 6, (60_000, 2)), rng.normal(-1.0, 0.02, 60_000)]
    box = rng.uniform([-1.5, -1.5, -1.0], [1.5, 1.5, 1.5], (50_000, 3))
    wall = np.c_[np.full(8_000, 3.0) + rng.normal(0, 0.01, 8_000), rng.uniform(-4, 4, 8_000),
                 rng.uniform(-1, 2, 8_000)]
    iso = rng.uniform([-6, -6, -1], [6, 6, 3], (300, 3))
    pts = np.concatenate([floor, box, wall, iso]).astype(np.float32)
    out = np.zeros((pts.shape[0], 4), np.float32)
    out[:, :3] = pts
    return out


@pytest.mark.parametrize("n_az,n_el", [(100, 37), (64, 3)])
def test_raycast_fan_clutter_and_odd_fans(oracle, n_az, n_el):
    """Fan sizes that are not multiples of the 64-lane wave (a ring spans waves, partial last
    wave), against a volumetric cloud; poses inside the box, at its edge, above, below the
    floor and far outside.  First hits, blocked counts and ray-hit tests bit-exact."""
    cloud = _clutter_cloud()
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        poses = np.array([[0.0, 0.0, 0.2, 0.0, 0.3], [1.5, -1.5, 1.5, 0.0, -2.0],
                          [-4.0, 2.0, 2.5, 0.0, 1.0], [0.5, 4.0, -1.5, 0.0, 0.0],
                          [40.0, 40.0, 0.0, 0.0, 0.0], [2.9, 0.0, 0.5, 0.0, 3.1]])
        fan = _abi.fan_params(n_az=n_az, n_el=n_el)
        blocked, units, fh, best = ctx.raycast_fan(poses, fan, want_first_hit=True)
        T = oracle.Cloud(cloud)
        r_blocked, r_units, r_fh = oracle.raycast_fan(T, poses, n_az, n_el, fan.el_min,
                                                      fan.el_max, fan.max_distance)
        np.testing.assert_array_equal(fh, r_fh)
        np.testing.assert_array_equal(blocked, r_blocked)
        np.testing.assert_array_equal(units, r_units)
        assert best == int(np.argmin(r_blocked))
        assert blocked[4] == 0 and blocked[0] > 0
    finally:
        ctx.close()


_CLUTTER_POSES = np.array([[0.0, 0.0, 0.2, 0.0, 0.3], [1.5, -1.5, 1.5, 0.0, -2.0],
                           [-4.0, 2.0, 2.5, 0.0, 1.0], [0.5, 4.0, -1.5, 0.0, 0.0],
                           [40.0, 40.0, 0.0, 0.0, 0.0], [2.9, 0.0, 0.5, 0.0, 3.1]])
_clutter_refs = {}


def _clutter_reference(oracle, n_az, n_el, n_poses):
    """The oracle's fan over _clutter_cloud() for the poses of
    test_raycast_fan_clutter_and_odd_fans (resized cyclically to n_poses), computed once."""
    key = (n_az, n_el, n_poses)
    if key not in _clutter_refs:
        poses = np.resize(_CLUTTER_POSES, (n_poses, 5))
        fan = _abi.fan_params(n_az=n_az, n_el=n_el)
        if "cloud" not in _clutter_refs:
            _clutter_refs["cloud"] = _clutter_cloud()
        T = oracle.Cloud(_clutter_refs["cloud"])
        r = oracle.raycast_fan(T, poses, n_az, n_el, fan.el_min, fan.el_max, fan.max_distance)
        for a in r:
            a.setflags(write=False)
        _clutter_refs[key] = (poses, fan) + tuple(r)
    return (_clutter_refs["cloud"],) + _clutter_refs[key]


@pytest.mark.parametrize("n_az,n_el", [(100, 37), (64, 3)])
@pytest.mark.parametrize("variant", ["1", "2", "4"])
def test_raycast_fan_batch_variants(oracle, monkeypatch, variant, n_az, n_el):
    """The A/B launches of PCP_FAN_BATCH (1 the pose-major grid of 128-thread
    blocks, 2 the occupancy-bit probe, 4 plain pose interleaving) on the clutter cloud of
    test_raycast_fan_clutter_and_odd_fans: its six poses, and eight of them (a whole number of
    XCD pose chunks).  The variable is read when the context is created (variant 2 builds its
    occupancy bits in set_terrain).  First hits, blocked counts and ray-hit tests bit-exact."""
    monkeypatch.setenv("PCP_FAN_BATCH", variant)
    ctx = _abi.Context(0)
    try:
        for n_poses in (6, 8):
            cloud, poses, fan, r_blocked, r_units, r_fh = _clutter_reference(oracle, n_az, n_el,
                                                                              n_poses)
            if n_poses == 6:
                ctx.set_terrain(cloud)
            blocked, units, fh, best = ctx.raycast_fan(poses, fan, want_first_hit=True)
            np.testing.assert_array_equal(fh, r_fh)
            np.testing.assert_array_equal(blocked, r_blocked)
            np.testing.assert_array_equal(units, r_units)
            assert best == int(np.argmin(r_blocked))
            assert blocked[4] == 0 and blocked[0] > 0
    finally:
        ctx.close()


def test_raycast_fan_stamps_mode(oracle):
    """pcp_raycast_fan_stamps (the wave-lifetime diagnostic: the interleaved kernels on the full
    grid) on the 64 x 3 fan over the clutter cloud, eight poses: four clock stamps in every
    (pose, wave) slot, in order; the plain query after it gives what the one before it gave."""
    cloud, poses, fan, r_blocked, r_units, r_fh = _clutter_reference(oracle, 64, 3, 8)
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        before = ctx.raycast_fan(poses, fan, want_first_hit=True)
        st = ctx.raycast_fan_stamps(poses, fan)
        after = ctx.raycast_fan(poses, fan, want_first_hit=True)
    finally:
        ctx.close()
    assert st.shape == (8, (64 * 3 + 63) // 64, 4) and st.dtype == np.uint64
    assert (st[..., 0] > 0).all()   # every slot written (the buffer starts zeroed)
    assert (st[..., 0] <= st[..., 1]).all() and (st[..., 1] <= st[..., 2]).all()
    assert (st[..., 2] <= st[..., 3]).all()
    for b, a in zip(before, after):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    np.testing.assert_array_equal(before[2], r_fh)
    np.testing.assert_array_equal(before[0], r_blocked)
    np.testing.assert_array_equal(before[1], r_units)


@pytest.mark.parametrize("dz,skip", [(3000.0, "1"), (-2500.0, "1"), (3000.0, "2"),
                                     (-2500.0, "2")])
def test_raycast_fan_far_from_origin(oracle, scene, cells, dz, skip, monkeypatch):
    """The terrain and the poses shifted by kilometres in z, where float spacing (~2.4e-4 m)
    exceeds the fixed 1e-4 m margins: the split-record walk skip widens its margin with |z|
    (pcp_march.hpp), so first hits, blocked counts and ray-hit tests stay exact on the
    fine-window copy (built at the first query), with one or two skip thresholds."""
    monkeypatch.setenv("PCP_TERRAIN_BLOCKS", "2")
    monkeypatch.setenv("PCP_FINE_SKIP", skip)
    terr = np.ascontiguousarray(scene.terrain.copy())
    terr[:, 2] += np.float32(dz)
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(terr, point_step=32)
        p = _abi.default_vl_params(num_candidates=100)
        g = _abi.Context(0)
        try:
            g.set_terrain(scene.terrain, point_step=32)
            poses = g.generate_candidates(cells.grid_bbox, p, scene.zx120_pose5)[::9][:8].copy()
        finally:
            g.close()
        poses[:, 2] += dz
        fan = _abi.fan_params(n_az=256, n_el=64)
        blocked, units, fh, _ = ctx.raycast_fan(poses, fan, want_first_hit=True)
        assert ctx.terrain_info()["scan_layout"] == "fine"
    finally:
        ctx.close()
    oracle.set_threads(8)
    r_blocked, r_units, r_fh = oracle.raycast_fan(oracle.Cloud(terr), poses, 256, 64,
                                                  fan.el_min, fan.el_max, fan.max_distance)
    oracle.set_threads(1)
    np.testing.assert_array_equal(fh, r_fh)
    np.testing.assert_array_equal(blocked, r_blocked)
    np.testing.assert_array_equal(units, r_units)
    assert blocked.sum() > 0


def test_raycast_fan_without_terrain_and_empty(oracle):
    """No terrain tree: every ray runs to the end unblocked (the reference's visible = true);
    zero poses: nothing to do, best index -1; an all-NaN terrain: an empty tree."""
    ctx = _abi.Context(0)
    try:
        fan = _abi.fan_params(n_az=128, n_el=16)
        poses = np.array([[0.0, 0.0, 1.0, 0.0, 0.0], [3.0, 1.0, 2.0, 0.0, 1.0]])
        K = len(_abi.step_table(fan.max_distance - 0.08))
        blocked, units, _, best = ctx.raycast_fan(poses, fan)
        assert blocked.tolist() == [0, 0] and units.tolist() == [128 * 16 * K] * 2
        assert best == 0
        b0, u0, _, best0 = ctx.raycast_fan(np.zeros((0, 5)), fan)
        assert b0.size == 0 and u0.size == 0 and best0 == -1
        nan_cloud = np.full((1000, 4), np.nan, np.float32)
        ctx.set_terrain(nan_cloud)
        blocked, units, fh, _ = ctx.raycast_fan(poses, fan, want_first_hit=True)
        assert blocked.tolist() == [0, 0] and (fh == -1).all()
    finally:
        ctx.close()


def test_raycast_fan_full_c2_workload(gpu, oracle, loaded, scene):
    """The whole headline workload of bench.py (BASELINE configs[1]: 256 candidate poses x the
    1024 x 256 fan on the 1M-point terrain), every first hit bit-exact against the oracle
    (67 M rays; the oracle's OpenMP build takes a few seconds on the box's 16 cores)."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import bench

    T, _ = loaded
    poses, _ = bench._poses_for(gpu, bench._grid_bbox(scene.area), scene.zx120_pose5, 256)
    fan = _abi.fan_params()
    blocked, units, fh, best = gpu.raycast_fan(poses, fan, want_first_hit=True)
    oracle.set_threads(16)
    try:
        r_blocked, r_units, r_fh = oracle.raycast_fan(T, poses, 1024, 256, fan.el_min,
                                                      fan.el_max, fan.max_distance)
    finally:
        oracle.set_threads(1)
    assert np.array_equal(blocked, r_blocked) and np.array_equal(units, r_units)
    bad = np.count_nonzero(fh != r_fh)
    assert bad == 0, f"{bad} of {fh.size} first hits differ"
    assert best == int(np.argmin(r_blocked))


def test_c4_sharded_4096_poses(gpu, oracle, loaded, scene):
    """BASELINE configs[3]: 4096 candidate poses split into 8 contiguous shards of 512 (one
    per GPU of the 8-GPU node), each shard through pcp_raycast_fan, combined as the RCCL
    all-reduce(MIN) combines them (dist.reduce_fan key vectors, elementwise min).  Blocked
    counts and ray-hit tests of all 4096 poses and the best index against the oracle; first
    hits bit-exact for every 4th pose of EVERY shard (1,024 poses x 262,144 rays)."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import bench
    from pointcloud_processor_amd import dist as pd

    T, _ = loaded
    P, G = 4096, 8
    poses, _ = bench._poses_for(gpu, bench._grid_bbox(scene.area), scene.zx120_pose5, P)
    assert poses.shape == (P, 5)
    fan = _abi.fan_params()
    key = np.full(P, pd.INT64_MAX, np.int64)
    units = np.zeros(P, np.uint64)
    oracle.set_threads(16)
    try:
        for g in range(G):
            lo, hi = pd.shard(P, G, g)
            assert hi - lo == 512
            b, u, fh, _ = gpu.raycast_fan(poses[lo:hi], fan, want_first_hit=True)
            k, _ = pd.reduce_fan(b, lo, hi, P)          # this rank's contribution
            key = np.minimum(key, k)                      # = all_reduce(MIN) over the ranks
            units[lo:hi] = u
            sel = np.arange(lo, hi, 4)                    # 128 poses of the shard
            _, _, r_fh = oracle.raycast_fan(T, poses[sel], 1024, 256, fan.el_min, fan.el_max,
                                            fan.max_distance)
            bad = np.count_nonzero(fh[sel - lo] != r_fh)
            assert bad == 0, f"shard {g}: {bad} first hits differ"
            del fh, r_fh
        best = int(np.argmin(key))
        r_blocked, r_units, _ = oracle.raycast_fan(T, poses, 1024, 256, fan.el_min, fan.el_max,
                                                   fan.max_distance, want_first_hit=False)
    finally:
        oracle.set_threads(1)
    np.testing.assert_array_equal(key, r_blocked.astype(np.int64))
    np.testing.assert_array_equal(units, r_units)
    assert best == int(np.argmin(r_blocked))


def test_terrain_replaced_after_block_copy(oracle, small_scene, scene):
    """set_terrain(A), two fan queries (the second builds A's block-major copy), then
    set_terrain(B) and a query: B's results must match the oracle on B (no stale copy or z
    bands of A paired with B's grid)."""
    ctx = _abi.Context(0)
    try:
        fan = _abi.fan_params(n_az=256, n_el=32)
        poses = np.array([[1.0, 0.5, 1.5, -0.3, 0.4], [6.0, -2.0, 1.2, -0.4, 2.5]])
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.raycast_fan(poses, fan)
        ctx.raycast_fan(poses, fan)
        B = small_scene.terrain
        ctx.set_terrain(B, point_step=32)
        for _ in range(3):   # before and after B's own block copy
            blocked, units, fh, _ = ctx.raycast_fan(poses, fan, want_first_hit=True)
            r_b, r_u, r_fh = oracle.raycast_fan(oracle.Cloud(B), poses, 256, 32, fan.el_min,
                                                fan.el_max, fan.max_distance)
            np.testing.assert_array_equal(fh, r_fh)
            np.testing.assert_array_equal(blocked, r_b)
            np.testing.assert_array_equal(units, r_u)
    finally:
        ctx.close()


def _rel_close(a, b):
    """The totals' loose parity bar (tests/parity.py: totals_match): every value within 2 ulps of
    the oracle's and at most max(2, 5 %) of them not bit-identical.  The censused cases (the
    91-candidate tick, the C5 frames, the long-range scene) use the exact bar instead."""
    return parity.totals_match(a, b)


PERTURB_LIB = Path(__file__).resolve().parents[1] / "pointcloud_processor_amd" / "_lib" / \
    "perturb" / "libpcp.so"
PERTURB8_LIB = Path(__file__).resolve().parents[1] / "pointcloud_processor_amd" / "_lib" / \
    "perturb8" / "libpcp.so"


def test_parity_bar_catches_one_ulp(oracle, loaded, scene, cells, aux):
    """The totals' bar is tight enough to see a one-ulp error in evaluateCellScore
    (virtual_lidar.cpp:689-700): the `make perturb` build (every cell score nextafter'd up, all
    else the production objects) fails it on the 91-candidate tick, the production build passes
    it on the same inputs, and the flags / covered counts / best index stay equal (only the
    totals' bits can show such an error)."""
    assert PERTURB_LIB.exists() and PERTURB8_LIB.exists(), \
        "build first (__graft_entry__.build(): make perturb perturb8)"
    T, A = loaded
    params = _abi.default_vl_params()
    res = {}
    for tag, path in (("prod", None), ("perturbed", str(PERTURB_LIB)),
                      ("perturbed8", str(PERTURB8_LIB))):
        with _abi.Context(0, lib_path=path) as ctx:
            ctx.set_terrain(scene.terrain, point_step=32)
            ctx.set_aux_cloud(aux, point_step=32)
            ctx.set_cells(cells.xyz, cells.normals)
            poses = ctx.generate_candidates(cells.grid_bbox, params, scene.zx120_pose5)
            fl = np.zeros(cells.xyz.shape[0], np.uint8)
            tot, cov, rep = ctx.score_poses(poses, scene.zx120_pose5, params, fl)
            res[tag] = (poses, tot, cov, rep.best_idx, fl)
    poses = res["prod"][0]
    r_tot, r_cov, r_rep = oracle.score_poses(T, A, cells.xyz, cells.normals, poses,
                                             scene.zx120_pose5, oracle.vl_params(),
                                             np.zeros(cells.xyz.shape[0], np.uint8))
    prod = parity.totals_report(res["prod"][1], r_tot)
    print("parity bar: production", prod)
    parity.assert_totals_exact(res["prod"][1], r_tot)   # 0 of 91 differ
    for tag in ("perturbed", "perturbed8"):   # every cell / every 8th cell one ulp up
        bad = parity.totals_report(res[tag][1], r_tot)
        print("parity bar:", tag, bad)
        assert not parity.totals_exact(res[tag][1], r_tot), (tag, bad)
        # (this tick's drifts are large enough for the loose bar as well: 61 and 10 of 91)
        assert not parity.totals_match(res[tag][1], r_tot), (tag, bad)
        np.testing.assert_array_equal(res[tag][2], r_cov)
        assert res[tag][3] == r_rep.best_idx == res["prod"][3]


def test_score_poses_matches_reference_loop(gpu, oracle, loaded, scene, cells):
    T, A = loaded
    params = _abi.default_vl_params()
    poses = gpu.generate_candidates(cells.grid_bbox, params, scene.zx120_pose5)
    assert len(poses) == 91
    flags_g = np.zeros(cells.xyz.shape[0], np.uint8)
    flags_r = flags_g.copy()
    tot, cov, rep = gpu.score_poses(poses, scene.zx120_pose5, params, flags_g)
    r_tot, r_cov, r_rep = oracle.score_poses(T, A, cells.xyz, cells.normals, poses,
                                             scene.zx120_pose5, oracle.vl_params(), flags_r)
    np.testing.assert_array_equal(flags_g, flags_r)
    np.testing.assert_array_equal(cov, r_cov)
    print("91-candidate tick totals", parity.totals_report(tot, r_tot))
    parity.assert_totals_exact(tot, r_tot)
    gd, rd = rep.as_dict(), r_rep.as_dict()
    for k in gd:
        if k in ("best_score", "zx120_total_score"):
            parity.assert_totals_exact(gd[k], rd[k])
        else:
            assert gd[k] == rd[k], k
    srt = np.sort(r_tot)[::-1]
    assert (srt[0] - srt[1]) > 1e-9 * srt[0]     # the argmax is decidable at this tolerance
    # a second tick starts from the stale flags (GridCell state persists between ticks)
    tot2, _, rep2 = gpu.score_poses(poses[::-1].copy(), scene.zx120_pose5, params, flags_g)
    r_tot2, _, r_rep2 = oracle.score_poses(T, A, cells.xyz, cells.normals, poses[::-1].copy(),
                                           scene.zx120_pose5, oracle.vl_params(), flags_r)
    np.testing.assert_array_equal(flags_g, flags_r)
    assert rep2.best_idx == r_rep2.best_idx


@pytest.mark.parametrize("wide", ["1", "0"])
@pytest.mark.parametrize("npose", [1, 3])
def test_score_few_poses_wide_lanes(oracle, scene, cells, aux, wide, npose, monkeypatch):
    """Few rays (C1 / C5 score one candidate): k_score_cells_wide splits each ray's samples
    over 16 lanes and ANDs their verdicts.  Same flags, coverage, totals and best pose as the
    reference loop, with the wide kernel on (default) and off (PCP_SCORE_WIDE=0)."""
    monkeypatch.setenv("PCP_SCORE_WIDE", wide)
    params = _abi.default_vl_params()
    T, A = oracle.Cloud(scene.terrain), oracle.Cloud(aux)
    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.set_aux_cloud(aux, point_step=32)
        ctx.set_cells(cells.xyz, cells.normals)
        poses = ctx.generate_candidates(cells.grid_bbox, params, scene.zx120_pose5)[:npose]
        assert (npose + 1) * cells.xyz.shape[0] <= 1 << 15   # the wide kernel's range
        fg = np.zeros(cells.xyz.shape[0], np.uint8)
        fr = fg.copy()
        tot, cov, rep = ctx.score_poses(poses, scene.zx120_pose5, params, fg)
        r_tot, r_cov, r_rep = oracle.score_poses(T, A, cells.xyz, cells.normals, poses,
                                                 scene.zx120_pose5, oracle.vl_params(), fr)
        np.testing.assert_array_equal(fg, fr)
        np.testing.assert_array_equal(cov, r_cov)
        assert _rel_close(tot, r_tot), np.max(np.abs(tot - r_tot))
        assert rep.best_idx == r_rep.best_idx
        assert rep.as_dict()["total_cells"] == r_rep.as_dict()["total_cells"]


def test_generate_and_score_matches_two_calls(gpu, loaded, scene, cells):
    """pcp_generate_and_score (one round trip: the scoring reads the candidates and their count
    where the generation left them) against pcp_generate_candidates + pcp_score_poses on the
    same context: poses, totals, covered counts, flags and the report bit-identical over ticks
    whose flags carry over, lattice sizes that change between calls, and a context without
    cells."""
    fa = np.zeros(cells.xyz.shape[0], np.uint8)
    fb = fa.copy()
    for nc in (None, 400, 100, None):
        params = _abi.default_vl_params() if nc is None else _abi.default_vl_params(num_candidates=nc)
        poses = gpu.generate_candidates(cells.grid_bbox, params, scene.zx120_pose5)
        tot, cov, rep = gpu.score_poses(poses, scene.zx120_pose5, params, fa)
        p2, tot2, cov2, rep2 = gpu.generate_and_score(cells.grid_bbox, params, scene.zx120_pose5, fb)
        np.testing.assert_array_equal(p2, poses)
        np.testing.assert_array_equal(tot2.view(np.uint64), tot.view(np.uint64))
        np.testing.assert_array_equal(cov2, cov)
        np.testing.assert_array_equal(fb, fa)
        assert rep2.as_dict() == rep.as_dict()
    with _abi.Context(0) as ctx:   # no cells, no terrain: the zeroed report, flat candidates
        params = _abi.default_vl_params(num_candidates=9)
        f0 = np.zeros(0, np.uint8)
        poses = ctx.generate_candidates(cells.grid_bbox, params, scene.zx120_pose5)
        tot, cov, rep = ctx.score_poses(poses, scene.zx120_pose5, params, f0)
        p2, tot2, cov2, rep2 = ctx.generate_and_score(cells.grid_bbox, params, scene.zx120_pose5, f0)
        np.testing.assert_array_equal(p2, poses)
        np.testing.assert_array_equal(tot2, tot)
        assert rep2.as_dict() == rep.as_dict()


def test_score_fov_boundary(oracle):
    """The FOV decision (virtual_lidar.cpp:665-672, |elevation - pitch| <= fov / 2) at and around
    its boundary: cells straight below and above a pose (elevation exactly -pi/2, +pi/2) and a
    hair off the vertical, pitches 0, +-1e-7, +-3e-6 (inside the band the kernel settles with
    the double atan2) and +-2e-5, +-1e-3 (settled by its float atan2).  No terrain: every cell
    in range and in view is visible, so the flags carry the FOV bits.  Flags, covered counts
    and totals against the oracle."""
    xyz = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 4.0], [1e-6, 0.0, 0.0], [0.0, -1e-4, 0.0],
                    [0.01, 0.0, 0.0], [0.0, 0.0, 0.5], [3.0, 0.0, 2.0], [0.0, 1e-7, 4.0],
                    [-2.0, 1.0, -3.0]])
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (xyz.shape[0], 1))
    pitches = [0.0, 1e-7, -1e-7, 3e-6, -3e-6, 2e-5, -2e-5, 1e-3, -1e-3]
    poses = np.array([[0.0, 0.0, 2.0, pt, 0.4] for pt in pitches])
    zx = np.array([0.0, 0.0, 2.0, 1e-7, 0.0])
    params = _abi.default_vl_params()
    with _abi.Context(0) as ctx:
        ctx.set_cells(xyz, nrm)
        fg = np.zeros(xyz.shape[0], np.uint8)
        fr = fg.copy()
        for tick in range(2):   # each pose alone: the flags show every pose's own bits
            for k in range(len(pitches)):
                tot, cov, rep = ctx.score_poses(poses[k:k + 1].copy(), zx, params, fg)
                r_tot, r_cov, r_rep = oracle.score_poses(None, None, xyz, nrm, poses[k:k + 1],
                                                         zx, oracle.vl_params(), fr)
                np.testing.assert_array_equal(fg, fr)
                np.testing.assert_array_equal(cov, r_cov)
                assert _rel_close(tot, r_tot)
                assert rep.green == r_rep.green and rep.yellow == r_rep.yellow
    # both sides of the boundary occur (the same double expression, in numpy)
    d = xyz[None, :, :] - poses[:, None, :3]
    L = np.linalg.norm(d, axis=2)
    ediff = np.arctan2(d[..., 2], np.hypot(d[..., 0], d[..., 1])) - poses[:, 3:4]
    fov = np.abs(ediff) <= (180.0 * np.pi / 180.0) / 2.0
    inr = (L >= 0.5) & (L <= params.max_distance)
    assert (inr & fov).any() and (inr & ~fov).any()


def test_score_poses_clutter(oracle):
    """Reference-mode scoring against the volumetric cloud: visibility marches that end at the
    cell (s_k < L - 0.08), cells inside the clutter, behind the wall and in the open."""
    cloud = _clutter_cloud(23)
    rng = np.random.default_rng(5)
    xyz = np.c_[rng.uniform(-5, 5, (400, 2)), rng.uniform(-1, 1.5, 400)]
    nrm = rng.normal(size=(400, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(cloud)
        ctx.set_cells(xyz, nrm)
        params = _abi.default_vl_params()
        poses = np.array([[0.0, 0.0, 2.5, -0.6, 0.0], [-4.0, -4.0, 1.0, -0.2, 0.8],
                          [4.5, 0.0, 0.5, 0.0, 3.1], [0.0, 5.0, 3.0, -1.2, -1.57]])
        zx = np.array([-5.0, 5.0, 2.0, -0.5, -0.7])
        flags_g = np.zeros(400, np.uint8)
        flags_r = flags_g.copy()
        tot, cov, rep = ctx.score_poses(poses, zx, params, flags_g)
        T = oracle.Cloud(cloud)
        r_tot, r_cov, r_rep = oracle.score_poses(T, None, xyz, nrm, poses, zx, oracle.vl_params(),
                                                 flags_r)
        np.testing.assert_array_equal(flags_g, flags_r)
        np.testing.assert_array_equal(cov, r_cov)
        assert _rel_close(tot, r_tot)
        assert rep.best_idx == r_rep.best_idx
        assert 0 < cov.min() and cov.max() < 400
    finally:
        ctx.close()


def test_score_poses_sparse_terrain(oracle):
    """A sparse terrain (a few thousand points over 40 m x 40 m, like the chain's carved
    terrain) takes the sparse z-band build and the coarse occupancy map that the cell march
    reads from LDS before each probe: flags and covered counts exact, totals within the parity bar,
    against the oracle.  Pillars between the poses and the cells make some rays blocked."""
    rng = np.random.default_rng(11)
    ground = np.c_[rng.uniform(-20, 20, (2_500, 2)), rng.normal(0.0, 0.05, 2_500)]
    pillars = [np.c_[x + rng.normal(0, 0.05, 300), y + rng.normal(0, 0.05, 300),
                     rng.uniform(0.0, 3.0, 300)] for x, y in ((3.0, 2.0), (-4.0, 5.0), (6.0, -6.0),
                                                            (0.5, 0.5))]
    pts = np.concatenate([ground] + pillars).astype(np.float32)
    cloud = np.zeros((pts.shape[0], 4), np.float32)
    cloud[:, :3] = pts
    xyz = np.c_[rng.uniform(-8, 8, (400, 2)), rng.uniform(-0.3, 0.6, 400)]
    nrm = rng.normal(size=(400, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    poses = np.array([[0.0, 0.0, 2.5, -0.6, 0.0], [-6.0, -6.0, 1.5, -0.3, 0.8],
                      [7.0, 1.0, 3.0, -0.9, 3.1], [1.0, 7.0, 1.2, 0.0, -1.57]])
    zx = np.array([-9.0, 9.0, 2.0, -0.5, -0.7])
    params = _abi.default_vl_params()
    with _abi.Context(0) as ctx:
        ctx.set_terrain(cloud)
        ctx.set_cells(xyz, nrm)
        fg = np.zeros(400, np.uint8)
        fr = fg.copy()
        T = oracle.Cloud(cloud)
        for tick in range(2):
            tot, cov, rep = ctx.score_poses(poses, zx, params, fg)
            r_tot, r_cov, r_rep = oracle.score_poses(T, None, xyz, nrm, poses, zx,
                                                     oracle.vl_params(), fr)
            np.testing.assert_array_equal(fg, fr)
            np.testing.assert_array_equal(cov, r_cov)
            assert _rel_close(tot, r_tot)
            assert rep.best_idx == r_rep.best_idx
        info = ctx.terrain_info()
        assert info["dims"][0] * info["dims"][1] * info["dims"][2] > 32 * cloud.shape[0]   # sparse
        assert cov.max() > 0


def test_score_poses_edge_states(oracle, scene, cells, aux):
    """No terrain (visible), no aux cloud, zero poses, zero cells, stale terrain tree."""
    params = _abi.default_vl_params(max_distance=12.0)
    zx = scene.zx120_pose5
    poses = np.array([[8.0, -3.0, 1.1, -0.3, 2.5], [0.0, 4.0, 1.1, -0.2, -1.0]])
    with _abi.Context(0) as ctx:
        # nothing loaded: every visibility check returns true (:721,:727)
        ctx.set_cells(cells.xyz, cells.normals)
        fg = np.zeros(cells.xyz.shape[0], np.uint8)
        fr = fg.copy()
        t, c, rep = ctx.score_poses(poses, zx, params, fg)
        rt, rc, rrep = oracle.score_poses(None, None, cells.xyz, cells.normals, poses, zx,
                                          oracle.vl_params(max_distance=12.0), fr)
        np.testing.assert_array_equal(fg, fr)
        np.testing.assert_array_equal(c, rc)
        assert _rel_close(t, rt)
        # zero poses: stats only, best -1
        t, c, rep = ctx.score_poses(np.zeros((0, 5)), zx, params, fg)
        assert rep.best_idx == -1 and t.size == 0 and rep.total_cells == cells.xyz.shape[0]
        # terrain then an empty terrain: ray casts keep the stale index, ground height sees
        # the empty cloud (0.0)
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.set_terrain(np.zeros((0, 8), np.float32), point_step=32)
        g = ctx.generate_candidates(cells.grid_bbox, params, zx)
        T = oracle.Cloud(scene.terrain)
        r = oracle.generate_candidates(T, cells.grid_bbox, oracle.vl_params(max_distance=12.0),
                                       zx, terrain_empty=True)
        np.testing.assert_array_equal(g[:, :3], r[:, :3])
        fg[:] = 0
        fr[:] = 0
        t, c, rep = ctx.score_poses(poses, zx, params, fg)
        rt, rc, rrep = oracle.score_poses(T, None, cells.xyz, cells.normals, poses, zx,
                                          oracle.vl_params(max_distance=12.0), fr)
        np.testing.assert_array_equal(fg, fr)
        np.testing.assert_array_equal(c, rc)
        # zero cells
        ctx.set_cells(np.zeros((0, 3)), np.zeros((0, 3), np.float32))
        t, c, rep = ctx.score_poses(poses, zx, params, np.zeros(0, np.uint8))
        assert rep.best_idx == 0 and np.all(t == 0)


# ---------------------------------------------------------------- excavation-area setup
def _normals_equal(got, ref):
    """Bit-identical normals, NaN where the reference has NaN (< 3 neighbours, non-finite)."""
    fin = np.isfinite(ref).all(1)
    assert np.array_equal(np.isfinite(got).all(1), fin)
    np.testing.assert_array_equal(got[fin].view(np.uint32), ref[fin].view(np.uint32))


@pytest.mark.parametrize("mode", ["exact", "exact_ordered", "exact_two_builds", "fixed"])
def test_excavation_area_setup(oracle, scene, mode, monkeypatch):
    """pcp_set_excavation_area against the oracle: grid bounds and the valid cells (positions,
    reference loop order) bit-exact.  Default path (PCP_NORMALS_EXACT=1): point normals and cell
    normals BIT-IDENTICAL -- PCL's float covariance sums in FLANN's (distance, index) order,
    eigen33 with glibc's float libm restated (pcp_libm.h), the cells' double sums where their
    order cannot change them in any order (k_cell_sums_exact), the others in FLANN's order;
    exact_ordered (PCP_CELLS_ORDER_FREE=0) sends every cell through the ordered lists;
    exact_two_builds builds the area's two grids separately (PCP_INDEX_PAIR=0).  The
    order-free fixed-point A/B kernels (PCP_NORMALS_EXACT=0): point normals within 2e-3, cells
    within 1e-4.  An empty area keeps the previous cells (virtual_lidar.cpp:168)."""
    exact = "0" if mode == "fixed" else "1"
    monkeypatch.setenv("PCP_NORMALS_EXACT", exact)
    # exact_two_builds: the area's two grids by two build_index calls + k_area_prep instead of
    # the paired build (PCP_INDEX_PAIR=0)
    monkeypatch.setenv("PCP_INDEX_PAIR", "0" if mode == "exact_two_builds" else "1")
    monkeypatch.setenv("PCP_CELLS_ORDER_FREE", "0" if mode == "exact_ordered" else "1")
    d = np.load(GOLD / "excavation.npz")
    ctx = _abi.Context(0)
    try:
        for area, ref in ((d["area"], None), (scene.area, "full")):
            if ref is None:
                r_n, r_xyz, r_cn, r_bb = d["normals"], d["cells"], d["cell_normals"], d["grid_bbox"]
            else:
                r_n = oracle.area_normals(area, 1.5)
                r_xyz, r_cn, r_bb, _ = oracle.excavation_grid(area, 0.1, 10, r_n)
            bb, n = ctx.set_excavation_area(area, 0.1, 10, point_step=area.shape[1] * 4)
            np.testing.assert_array_equal(bb, r_bb)
            assert n == r_xyz.shape[0]
            xyz, cn = ctx.get_cells()
            np.testing.assert_array_equal(xyz, r_xyz)
            an = ctx.get_area_normals()
            if exact == "1":
                _normals_equal(an, r_n)
                np.testing.assert_array_equal(cn.view(np.uint32), r_cn.view(np.uint32))
            else:
                fin = np.isfinite(r_n).all(1)
                assert np.array_equal(np.isfinite(an).all(1), fin)
                np.testing.assert_allclose(an[fin], r_n[fin], atol=2e-3)
                np.testing.assert_allclose(cn, r_cn, atol=1e-4)
        bb, n2 = ctx.set_excavation_area(np.zeros((0, 4), np.float32), 0.1, 10)
        assert n2 == n and np.array_equal(ctx.get_cells()[0], xyz)
    finally:
        ctx.close()


@pytest.mark.parametrize("order_free,small", [("1", "1"), ("0", "1"), ("1", "0")])
def test_excavation_area_normals_long_lists_and_ties(oracle, order_free, small, monkeypatch):
    """The exact normals where the neighbour lists pass the LDS sort (> 4,096 neighbours within
    1.5 m: sorted in global memory), with exact distance ties (a lattice, duplicated points: the
    reference's order breaks them by index), non-finite points (NaN normals, absent from every
    list) and isolated points (< 3 neighbours: NaN).  A plane tilted by 1e-6 beside it gives
    normals with components ~2^-20 of their largest: the cells near it fail
    k_cell_sums_exact's bound and take the ordered path in the same frame as the others.
    Point and cell normals bit-identical, cells order-free where exact (default) and all
    ordered (PCP_CELLS_ORDER_FREE=0); the lists' LDS keys with 16-bit indices (areas below 2^16
    points, default) and 32-bit (PCP_NB_SMALL=0, every larger area)."""
    monkeypatch.setenv("PCP_CELLS_ORDER_FREE", order_free)
    monkeypatch.setenv("PCP_NB_SMALL", small)
    rng = np.random.default_rng(11)
    g = np.arange(90) * 0.025
    X, Y = np.meshgrid(g, g)
    P = np.stack([X.ravel(), Y.ravel(), 0.3 * np.sin(X.ravel()) + rng.normal(0, 0.002, X.size)], 1)
    P[::7, 2] = np.round(P[::7, 2], 2)                        # many exact-distance ties
    t = np.arange(30) * 0.05
    TX, TY = np.meshgrid(4.0 + t, t)
    tilt = np.stack([TX.ravel(), TY.ravel(), 1e-6 * TX.ravel()], 1)   # tiny normal components
    P = np.concatenate([P, P[100:140], tilt, [[9.0, 9.0, 0.0], [9.5, 9.0, 0.1]]])   # dups, isolated
    a = np.zeros((P.shape[0], 4), np.float32)
    a[:, :3] = P
    a[rng.integers(0, a.shape[0], 6), 1] = np.nan
    r_n = oracle.area_normals(a, 1.5)
    r_xyz, r_cn, r_bb, _ = oracle.excavation_grid(a, 0.1, 4, r_n)
    with _abi.Context(0) as ctx:
        for _ in range(2):                                   # the regrown list buffer, reused
            bb, n = ctx.set_excavation_area(a, 0.1, 4)
            np.testing.assert_array_equal(bb, r_bb)
            assert n == r_xyz.shape[0]
            _normals_equal(ctx.get_area_normals(), r_n)
            xyz, cn = ctx.get_cells()
            np.testing.assert_array_equal(xyz, r_xyz)
            np.testing.assert_array_equal(cn.view(np.uint32), r_cn.view(np.uint32))


@pytest.mark.parametrize("region_pct,guess", [("10", None), ("100", "4096"), ("10", "4096"),
                                              ("75", "4096")])
def test_excavation_area_list_spill_pool(oracle, region_pct, guess, monkeypatch):
    """The neighbour lists' capacity paths (k_nb_lists): a list its block's region cannot hold
    spills to the shared pool behind the regions (PCP_NB_REGION_PCT=10: most lists spill), and a
    list that fits neither sets the overflow, after which the host regrows both buffers and runs
    the normals again (PCP_NB_GUESS_WORDS=4096: a first buffer far too small; 100: no pool, the
    regions alone).  Point and cell normals bit-identical to the oracle on every path, and the
    second setup of the same area reallocates nothing."""
    monkeypatch.setenv("PCP_NB_REGION_PCT", region_pct)
    if guess:
        monkeypatch.setenv("PCP_NB_GUESS_WORDS", guess)
    a = _long_list_area()
    r_n = oracle.area_normals(a, 1.5)
    r_xyz, r_cn, r_bb, _ = oracle.excavation_grid(a, 0.1, 4, r_n)
    with _abi.Context(0) as ctx:
        for rep in range(2):
            before = _abi.alloc_stats()["device"]
            bb, n = ctx.set_excavation_area(a, 0.1, 4)
            grew = _abi.alloc_stats()["device"] - before
            np.testing.assert_array_equal(bb, r_bb)
            assert n == r_xyz.shape[0]
            _normals_equal(ctx.get_area_normals(), r_n)
            xyz, cn = ctx.get_cells()
            np.testing.assert_array_equal(xyz, r_xyz)
            np.testing.assert_array_equal(cn.view(np.uint32), r_cn.view(np.uint32))
            if rep:
                assert grew == 0, grew


def _long_list_area():
    rng = np.random.default_rng(11)
    g = np.arange(90) * 0.025
    X, Y = np.meshgrid(g, g)
    P = np.stack([X.ravel(), Y.ravel(), 0.3 * np.sin(X.ravel()) + rng.normal(0, 0.002, X.size)], 1)
    P[::7, 2] = np.round(P[::7, 2], 2)
    a = np.zeros((P.shape[0], 4), np.float32)
    a[:, :3] = P
    return a


@pytest.mark.parametrize("which,guess", [("golden", None), ("long_lists", None),
                                         ("long_lists", "4096"), ("golden", "4096")])
def test_excavation_area_async_then_tick(oracle, scene, which, guess, monkeypatch):
    """pcp_set_excavation_area_async (the composed chain's grid setup: enqueued, not waited for)
    followed by the terrain and the tick (pcp_generate_and_score, which settles it after its own
    synchronisation -- and, on a fresh context whose first neighbour-list guess overflows, regrows
    the lists, reruns them and ticks again): poses, totals, covered counts, flags, the report and
    the cells bit-identical to the synchronous setup's; a second tick from the stale flags too;
    an async setup settled by pcp_get_cells gives the same cells.  PCP_NB_GUESS_WORDS=4096: the
    first list buffers far too small, so the tick finds the overflow after its wait (the setup
    ran on its side stream), regrows, reruns the normals and ticks again."""
    if guess:
        monkeypatch.setenv("PCP_NB_GUESS_WORDS", guess)
    area = np.load(GOLD / "excavation.npz")["area"] if which == "golden" else _long_list_area()
    params = _abi.default_vl_params(num_candidates=36)
    zx = np.array([0.4, 0.5, 3.5, -math.pi / 6, 0.0])
    out = {}
    for mode in ("sync", "async"):
        with _abi.Context(0) as ctx:
            ctx.set_terrain(scene.terrain, point_step=32)
            if mode == "sync":
                bb, n = ctx.set_excavation_area(area, 0.1, 10, point_step=area.shape[1] * 4)
                flags = np.zeros(max(n, 1), np.uint8)
            else:
                bb, cap = ctx.set_excavation_area_async(area, 0.1, 10, point_step=area.shape[1] * 4)
                flags = np.zeros(max(cap, 1), np.uint8)
            poses, tot, cov, rep = ctx.generate_and_score(bb, params, zx, flags)
            n = ctx.cells_count()
            fl1 = flags[:n].copy()
            poses2, tot2, cov2, rep2 = ctx.generate_and_score(bb, params, zx, fl1)
            xyz, cn = ctx.get_cells()
            out[mode] = (bb, n, poses, tot, cov, rep.as_dict(), fl1, tot2, rep2.as_dict(), xyz, cn)
            if mode == "async":   # an async setup settled by a reader of the cells
                ctx.set_excavation_area_async(area, 0.1, 10, point_step=area.shape[1] * 4)
                xyz3, cn3 = ctx.get_cells()
                np.testing.assert_array_equal(xyz3, xyz)
                np.testing.assert_array_equal(cn3.view(np.uint32), cn.view(np.uint32))
    a, b = out["sync"], out["async"]
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1] == b[1] and a[1] > 0
    for i in (2, 3, 4, 6, 7, 9):
        np.testing.assert_array_equal(np.asarray(a[i]).view(np.uint8), np.asarray(b[i]).view(np.uint8))
    np.testing.assert_array_equal(a[10].view(np.uint32), b[10].view(np.uint32))
    assert a[5] == b[5] and a[8] == b[8]


def test_excavate_area_async_matches_three_calls():
    """pcp_excavate_area_async (the carve node and virtual_lidar's area + terrain callbacks
    composed: the carve's landed records feed the grid setup and the terrain index in place)
    against pcp_excavate + pcp_set_excavation_area + pcp_set_terrain on the same merged cloud:
    both messages, the pose, the grid bounds, the cells and their normals, and a tick's poses,
    totals, covered counts, flags and report bit-identical.  Three frames in a row on one
    context (the landing is reused while the previous setup is pending: the call settles it
    first), the third with the carve moved (a new generated lattice).  "landed": the composed
    call with null outputs, the messages read in place (pcp_excavate_landed) after the zx120
    index and the tick -- the same bytes."""
    box = np.array([0.0, 15.0, -10.0, 10.0, -1.5, 10.0])
    tfs = [((8.0, -3.0, 2.0), (0.0, 0.0, 0.2588190451025208, 0.9659258262890683)),
           ((0.55, 0.4, 3.5), (0.0, 0.21633, 0.0, 0.97632))]
    params = _abi.default_vl_params(num_candidates=36)
    zx = np.array([0.4, 0.5, 3.5, -math.pi / 6, 0.0])
    frames = []
    for f, (seed, base) in enumerate([(101, ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))),
                                      (131, ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))),
                                      (131, ((0.3, -0.2, 0.0), (0.0, 0.0, 0.0998, 0.9950)))]):
        scans = [synth.lidar_cloud(60_032, sensor_height=2.0, seed=seed),
                 synth.lidar_cloud(60_032, sensor_height=3.5, seed=seed + 1)]
        frames.append((scans, base))
    out = {}
    for mode in ("calls", "composed", "landed"):
        res = []
        with _abi.Context(0) as ctx:
            for scans, base in frames:
                filt = [ctx.crop_voxel(sc, box, 0.2)[0] for sc in scans]
                merged = ctx.transform_concat(filt, tfs, [(255, 0, 0), (0, 0, 255)])
                if mode == "calls":
                    terr, area, pose = ctx.excavate(merged, base)
                    bb, n = ctx.set_excavation_area_async(area, 0.1, 10, point_step=32)
                    ctx.set_terrain(terr, point_step=32)
                else:
                    terr, area, pose, bb, n = ctx.excavate_area_async(merged, base,
                                                                      landed=mode == "landed")
                    tp = ctypes.c_void_p()
                    rc = ctx.lib.pcp_excavate_landed(ctx.h, ctypes.byref(tp), None)
                    # left in place only by the null-output call
                    assert (rc == _abi.PCP_OK) == (mode == "landed"), rc
                ctx.set_aux_cloud(filt[1])
                flags = np.zeros(max(n, 1), np.uint8)
                poses, tot, cov, rep = ctx.generate_and_score(bb, params, zx, flags)
                nc = ctx.cells_count()
                xyz, cn = ctx.get_cells()
                res.append((terr.copy(), area.copy(), pose, bb, nc, poses, tot, cov, flags[:nc].copy(),
                            rep.as_dict(), xyz, cn))
        out[mode] = res
    for a, b, c in zip(out["calls"], out["composed"], out["landed"]):
        for i in (0, 1, 2, 3, 5, 6, 7, 8, 10, 11):
            np.testing.assert_array_equal(np.asarray(a[i]).view(np.uint8), np.asarray(b[i]).view(np.uint8))
            np.testing.assert_array_equal(np.asarray(a[i]).view(np.uint8), np.asarray(c[i]).view(np.uint8))
        assert a[4] == b[4] == c[4] and a[4] > 0
        assert a[9] == b[9] == c[9]


def test_excavation_area_async_back_to_back(scene):
    """Async grid setups in a row with no tick between them (each settles the one before it:
    its side stream joined, its lists checked), a terrain change and a zx120 cloud between
    setup and tick, then the tick: cells, normals, poses, totals, flags and report equal to a
    context that ran only the last setup synchronously."""
    d = np.load(GOLD / "excavation.npz")
    areas = [_long_list_area(), d["area"], _long_list_area()[::3].copy()]
    params = _abi.default_vl_params(num_candidates=25)
    zx = np.array([0.4, 0.5, 3.5, -math.pi / 6, 0.0])
    aux = scene.terrain[::50, :4].copy()
    out = []
    for mode in ("sync_last", "async_chain"):
        with _abi.Context(0) as ctx:
            ctx.set_terrain(scene.terrain[:1000], point_step=32)
            if mode == "sync_last":
                ctx.set_terrain(scene.terrain, point_step=32)
                bb, n = ctx.set_excavation_area(areas[-1], 0.1, 10, point_step=areas[-1].shape[1] * 4)
                flags = np.zeros(max(n, 1), np.uint8)
            else:
                for a in areas:
                    bb, cap = ctx.set_excavation_area_async(a, 0.1, 10, point_step=a.shape[1] * 4)
                ctx.set_terrain(scene.terrain, point_step=32)
                flags = np.zeros(max(cap, 1), np.uint8)
            ctx.set_aux_cloud(aux)
            poses, tot, cov, rep = ctx.generate_and_score(bb, params, zx, flags)
            n = ctx.cells_count()
            xyz, cn = ctx.get_cells()
            out.append((bb, n, poses, tot, cov, flags[:n].copy(), rep.as_dict(), xyz, cn))
    a, b = out
    assert a[1] == b[1] and a[1] > 0 and a[6] == b[6]
    for i in (0, 2, 3, 4, 5, 7, 8):
        np.testing.assert_array_equal(np.asarray(a[i]).view(np.uint8), np.asarray(b[i]).view(np.uint8))


def _degenerate_areas():
    rng = np.random.default_rng(23)
    out = {}
    out["three_points"] = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.01]])
    out["identical"] = np.concatenate([np.tile([[1.0, 2.0, 0.5]], (50, 1)),
                                       rng.uniform(0, 0.4, (30, 3)) + [1.0, 2.0, 0.3]])
    t = np.arange(200) * 0.01
    out["collinear"] = np.stack([t, 0.5 * t, 0.1 * t], 1)                 # rank-1 covariance
    g = np.arange(40) * 0.05
    X, Y = np.meshgrid(g, g)
    plane = np.stack([X.ravel(), Y.ravel(), 0.2 * X.ravel() + rng.normal(0, 0.003, X.size)], 1)
    out["far_from_origin"] = plane + [2000.0, -1500.0, 300.0]            # float spacing ~1e-4 m
    return out


@pytest.mark.parametrize("case", ["three_points", "identical", "collinear", "far_from_origin"])
def test_excavation_area_normals_degenerate(oracle, case):
    """Degenerate areas through the exact normals: three points (lists below PCL's minimum),
    50 identical points beside a few others (zero distances: the order is the index order, zero
    covariance), a line (rank-1 covariance: eigen33's degenerate branches), and a plane
    kilometres from the origin (coarse float spacing in the distances and the sums).  Point and
    cell normals and the cells bit-identical to the oracle."""
    P = _degenerate_areas()[case]
    a = np.zeros((P.shape[0], 4), np.float32)
    a[:, :3] = P
    r_n = oracle.area_normals(a, 1.5)
    r_xyz, r_cn, r_bb, _ = oracle.excavation_grid(a, 0.1, 4, r_n)
    with _abi.Context(0) as ctx:
        bb, n = ctx.set_excavation_area(a, 0.1, 4)
        np.testing.assert_array_equal(bb, r_bb)
        assert n == r_xyz.shape[0]
        _normals_equal(ctx.get_area_normals(), r_n)
        if n:
            xyz, cn = ctx.get_cells()
            np.testing.assert_array_equal(xyz, r_xyz)
            np.testing.assert_array_equal(cn.view(np.uint32), r_cn.view(np.uint32))


# ---------------------------------------------------------------- excavated-terrain carve
def _matched_cloud(seed=3):
    """A /matched_point_cloud stand-in: a noisy 0.05 m lattice (PointXYZRGB, 32 B), a raised
    block over the pit, a hole with a few points 0.8 m up (nearest-point fallbacks), NaNs."""
    rng = np.random.default_rng(seed)
    xs, ys = np.arange(-2.0, 9.0, 0.05), np.arange(-3.0, 6.0, 0.05)
    X, Y = np.meshgrid(xs, ys)
    P = np.stack([X.ravel(), Y.ravel(), rng.normal(0, 0.01, X.size)], 1)
    hole = np.hypot(P[:, 0] - 5.0, P[:, 1] - 0.0) < 0.8
    P = P[~hole]
    block = np.stack(np.meshgrid(np.arange(4.0, 4.6, 0.05), np.arange(1.0, 1.6, 0.05),
                                 np.array([0.3, 1.5])), -1).reshape(-1, 3)
    lifted = np.array([[5.0, 0.0, 0.8], [5.1, 0.2, 0.8], [4.8, -0.3, 0.85]])
    P = np.concatenate([P, block, lifted])
    c = np.zeros((P.shape[0], 8), np.float32)
    c[:, :3] = P
    c[:, 4] = np.frombuffer(np.full(P.shape[0], 0xFF00FF00, np.uint32).tobytes(), np.float32)
    c[rng.integers(0, P.shape[0], 20), 0] = np.nan
    return c


def test_excavate_matches_oracle(gpu, oracle):
    """pcp_excavate against the CPU restatement: kept points (order, bytes), the generated
    excavated surface and /excavation_area records, and the marker pose, all bit-exact.  The
    sequence covers the device copy of the generated lattice: reused for a new cloud under the
    same pose, regenerated for a new pose, and for a cloud that outgrows its buffer."""
    for seed, yaw_deg, twice in ((3, 20.0, False), (4, 20.0, False), (3, -35.0, False),
                                 (7, -35.0, True), (3, 20.0, False)):
        c = _matched_cloud(seed)
        if twice:
            c = np.concatenate([c, _matched_cloud(seed + 1)])
        yaw = math.radians(yaw_deg)
        t, q = (0.3, -0.2, 0.1), (0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2))
        terr, area, pose = gpu.excavate(c, (t, q))
        keep, surf, r_area, r_pose = oracle.excavate(c, t, q)
        np.testing.assert_array_equal(pose, r_pose)
        nk = int(keep.sum())
        assert 0 < nk < c.shape[0] and terr.shape[0] == nk + surf.shape[0]
        kept = c[keep]
        np.testing.assert_array_equal(terr[:nk, :3].view(np.uint32), kept[:, :3].view(np.uint32))
        np.testing.assert_array_equal(terr[:nk, 4].view(np.uint32), kept[:, 4].view(np.uint32))
        np.testing.assert_array_equal(terr[nk:, [0, 1, 2, 4]].view(np.uint32), surf.view(np.uint32))
        np.testing.assert_array_equal(area[:, [0, 1, 2, 4]].view(np.uint32), r_area.view(np.uint32))


@pytest.mark.parametrize("case", ["empty", "all_nan", "far", "rect", "dense_deep"])
def test_excavate_edge_cases(gpu, oracle, case):
    """pcp_excavate against the CPU restatement on the edges: an empty cloud, an all-NaN cloud,
    a cloud 200 m away from the pit (every height from the nearest-point fallback), the
    rectangle mode (l_shape_enabled 0) and a denser, deeper surface (point_density 0.1, depth
    0.5).  Kept points, generated surface, /excavation_area records and the marker pose
    bit-exact."""
    c = _matched_cloud(6)
    kw = {}
    if case == "empty":
        c = np.zeros((0, 8), np.float32)
    elif case == "all_nan":
        c[:, 0] = np.nan
    elif case == "far":
        c[:, 0] += 200.0
    elif case == "rect":
        kw = {"l_shape_enabled": 0}
    else:
        kw = {"point_density": 0.1, "depth": 0.5}
    yaw = math.radians(15.0)
    t, q = (0.3, -0.2, 0.1), (0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2))
    terr, area, pose = gpu.excavate(c, (t, q), _abi.excavation_params(**kw))
    keep, surf, r_area, r_pose = oracle.excavate(c, t, q, oracle.exc_params(**kw))
    np.testing.assert_array_equal(pose, r_pose)
    nk = int(keep.sum())
    assert terr.shape[0] == nk + surf.shape[0]
    kept = c[keep]
    np.testing.assert_array_equal(terr[:nk, :3].view(np.uint32), kept[:, :3].view(np.uint32))
    np.testing.assert_array_equal(terr[:nk, 4].view(np.uint32), kept[:, 4].view(np.uint32))
    np.testing.assert_array_equal(terr[nk:, [0, 1, 2, 4]].view(np.uint32), surf.view(np.uint32))
    np.testing.assert_array_equal(area[:, [0, 1, 2, 4]].view(np.uint32), r_area.view(np.uint32))


def test_excavate_bounds_hold(gpu):
    """pcp_excavate_bounds caps every output the carve can produce (rectangle and L modes)."""
    c = _matched_cloud(5)
    for kw in ({}, {"l_shape_enabled": 0}, {"point_density": 0.1, "depth": 0.5}):
        p = _abi.excavation_params(**kw)
        terr, area, _ = gpu.excavate(c, ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)), p)
        nt, na = C_u64(), C_u64()
        assert gpu.lib.pcp_excavate_bounds(C_ref(p), c.shape[0], C_ref(nt), C_ref(na)) == 0
        assert terr.shape[0] <= nt.value and area.shape[0] <= na.value


# ---------------------------------------------------------------- drivable-area grid
@pytest.mark.parametrize("kw", [{}, {"grid_resolution": 0.5, "map_width": 60.0, "map_height": 40.0,
                                     "min_points_per_cell": 3, "max_gradient": 0.2}])
def test_drivable_area_matches_oracle(gpu, oracle, kw):
    """calc_drivable_area (robotCloudCallback :67-226) against the CPU restatement: the int8
    occupancy grid and its origin bit-exact (start-clear disc, unknown, obstacle, free)."""
    rng = np.random.default_rng(11)
    n = 200_000
    c = np.zeros((n, 4), np.float32)
    c[:, 0] = rng.uniform(-45, 45, n)
    c[:, 1] = rng.uniform(-45, 45, n)
    c[:, 2] = rng.normal(-1.5, 0.05, n)
    steep = (c[:, 0] > 5) & (c[:, 0] < 15)
    c[steep, 2] += rng.uniform(0, 1.5, steep.sum())
    c[rng.integers(0, n, 50), 1] = np.nan
    yaw = math.radians(25.0)
    t, q = (3.0, -2.0, 1.8), (0.0, 0.05, math.sin(yaw / 2), math.cos(yaw / 2))
    p = _abi.drivable_params(**kw)
    grid, origin = gpu.drivable_area(c, (t, q), (3.0, -2.0), (1.0, 0.5), p)
    ref, r_origin = oracle.drivable_area(c, t, q, (3.0, -2.0), (1.0, 0.5), p.grid_resolution,
                                         p.map_width, p.map_height, p.max_gradient,
                                         p.min_points_per_cell, p.start_clear_radius)
    np.testing.assert_array_equal(origin, r_origin)
    np.testing.assert_array_equal(grid, ref)
    assert {-1, 0, 100} <= set(np.unique(grid).tolist())


@pytest.mark.parametrize("case", ["empty", "all_nan", "outside_map", "one_cell"])
def test_drivable_area_edge_cases(gpu, oracle, case):
    """calc_drivable_area on the edges: an empty cloud and an all-NaN one (only the start-clear
    disc is free; an empty cloud leaves the whole grid free, as the reference's), every point
    outside the map, and one column of points (a single cell, an obstacle by its z spread).
    Grid and origin bit-exact against the CPU restatement."""
    rng = np.random.default_rng(5)
    if case == "empty":
        c = np.zeros((0, 4), np.float32)
    else:
        n = 5_000
        c = np.zeros((n, 4), np.float32)
        c[:, 0] = rng.uniform(-2, 2, n)
        c[:, 1] = rng.uniform(-2, 2, n)
        c[:, 2] = rng.normal(-1.5, 0.05, n)
        if case == "all_nan":
            c[:, 0] = np.nan
        elif case == "outside_map":
            c[:, 0] += 500.0
        else:
            c[:, 0] = 4.0
            c[:, 1] = 6.0
    yaw = math.radians(-40.0)
    t, q = (1.0, 2.0, 1.8), (0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2))
    p = _abi.drivable_params(min_points_per_cell=3)
    grid, origin = gpu.drivable_area(c, (t, q), (1.0, 2.0), (0.0, 0.0), p)
    ref, r_origin = oracle.drivable_area(c, t, q, (1.0, 2.0), (0.0, 0.0), p.grid_resolution,
                                         p.map_width, p.map_height, p.max_gradient,
                                         p.min_points_per_cell, p.start_clear_radius)
    np.testing.assert_array_equal(origin, r_origin)
    np.testing.assert_array_equal(grid, ref)


# (PCP_TERRAIN_BLOCKS, PCP_TERRAIN_FINE) -> the layout the scans walk from the first query
# (PCP_TERRAIN_BLOCKS, PCP_TERRAIN_FINE, PCP_FINE_TILE, expected scan layout); fine tile 0:
# x-fastest 8-byte records, 1: 4 x 4 tiles of them, 2: split records (2-byte thresholds +
# 4-byte starts) in 8 x 8 tiles
# (the fine-window entries are 12-byte packed unless the tile field carries "u": PCP_FINE_PACK=0)
LAYOUTS = [("0", "3", "1", "cells"), ("2", "0", "1", "blocks"), ("2", "2", "1", "fine"),
           ("2", "3", "1", "fine"), ("2", "2", "0", "fine"), ("2", "2", "2", "fine"),
           ("2", "3", "2", "fine"), ("2", "2", "2u", "fine")]


@pytest.mark.parametrize("mode,fine,tile,layout", LAYOUTS)
def test_terrain_block_copy_paths(oracle, scene, cells, aux, mode, fine, tile, layout,
                                  monkeypatch):
    """PCP_TERRAIN_BLOCKS=0 scans the per-cell runs, =2 the block-major copy (PCP_TERRAIN_FINE=0:
    2x2x2 blocks, F > 0: windows of fine cells c / F) from the first query on (the default, 1,
    switches at the second query): all bit-exact on the fan and the reference-mode scoring."""
    monkeypatch.setenv("PCP_TERRAIN_BLOCKS", mode)
    monkeypatch.setenv("PCP_TERRAIN_FINE", fine)
    monkeypatch.setenv("PCP_FINE_TILE", tile.rstrip("u"))
    monkeypatch.setenv("PCP_FINE_PACK", "0" if tile.endswith("u") else "1")
    ctx = _abi.Context(0)
    try:
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.set_aux_cloud(aux, point_step=32)
        ctx.set_cells(cells.xyz, cells.normals)
        T, A = oracle.Cloud(scene.terrain), oracle.Cloud(aux)
        params = _abi.default_vl_params()
        poses = ctx.generate_candidates(cells.grid_bbox, params, scene.zx120_pose5)
        fan = _abi.fan_params(n_az=128, n_el=48)
        _, _, fh, _ = ctx.raycast_fan(poses[:5], fan, want_first_hit=True)
        assert ctx.terrain_info()["scan_layout"] == layout
        _, _, r_fh = oracle.raycast_fan(T, poses[:5], 128, 48, fan.el_min, fan.el_max,
                                        fan.max_distance)
        np.testing.assert_array_equal(fh, r_fh)
        flags_g = np.zeros(cells.xyz.shape[0], np.uint8)
        flags_r = flags_g.copy()
        tot, cov, rep = ctx.score_poses(poses, scene.zx120_pose5, params, flags_g)
        r_tot, r_cov, r_rep = oracle.score_poses(T, A, cells.xyz, cells.normals, poses,
                                                 scene.zx120_pose5, oracle.vl_params(), flags_r)
        np.testing.assert_array_equal(flags_g, flags_r)
        np.testing.assert_array_equal(cov, r_cov)
        assert _rel_close(tot, r_tot)
        assert rep.best_idx == r_rep.best_idx
    finally:
        ctx.close()


@pytest.mark.parametrize("mode,fine,tile,layout", LAYOUTS)
def test_terrain_block_copy_dense_and_tiny(oracle, mode, fine, tile, layout, monkeypatch):
    """Block-major copies on awkward terrains: 20 k points packed into a 0.3 m cube (blocks of
    thousands of points, ties in z) next to a sparse plane, and a one-point terrain."""
    monkeypatch.setenv("PCP_TERRAIN_BLOCKS", mode)
    monkeypatch.setenv("PCP_TERRAIN_FINE", fine)
    monkeypatch.setenv("PCP_FINE_TILE", tile.rstrip("u"))
    monkeypatch.setenv("PCP_FINE_PACK", "0" if tile.endswith("u") else "1")
    rng = np.random.default_rng(11)
    dense = np.column_stack([rng.uniform(2.0, 2.3, 20_000), rng.uniform(-0.15, 0.15, 20_000),
                             np.round(rng.uniform(0.0, 0.3, 20_000), 2)])
    gx, gy = np.meshgrid(np.arange(-3.0, 6.0, 0.07), np.arange(-3.0, 3.0, 0.07))
    plane = np.column_stack([gx.ravel(), gy.ravel(), rng.normal(-0.5, 0.01, gx.size)])
    poses = np.array([[0.0, 0.0, 1.0, -0.3, 0.0], [4.5, 0.5, 0.8, 0.0, np.pi],
                      [2.15, 0.0, 0.15, 0.0, 0.3], [-2.0, -2.0, 2.5, -0.8, 0.7]])
    fan = _abi.fan_params(n_az=96, n_el=40, el_min_deg=-80.0, el_max_deg=60.0, max_distance=9.0)
    for pts in (np.vstack([dense, plane]), np.array([[1.0, 0.2, 0.4]])):
        cloud = np.zeros((pts.shape[0], 8), np.float32)
        cloud[:, :3] = pts
        ctx = _abi.Context(0)
        try:
            ctx.set_terrain(cloud, point_step=32)
            for _ in range(2):   # mode 1 would switch paths between these two calls
                blocked, units, fh, _ = ctx.raycast_fan(poses, fan, want_first_hit=True)
                r_blocked, r_units, r_fh = oracle.raycast_fan(oracle.Cloud(cloud), poses, 96, 40,
                                                              fan.el_min, fan.el_max, 9.0)
                np.testing.assert_array_equal(fh, r_fh)
                np.testing.assert_array_equal(blocked, r_blocked)
                np.testing.assert_array_equal(units, r_units)
                assert ctx.terrain_info()["scan_layout"] == layout
        finally:
            ctx.close()


@pytest.mark.parametrize("skip", ["1", "2"])
def test_fine_copy_dense_window(oracle, monkeypatch, skip):
    """70,000 points in a 5 cm cube: fine windows of 70 k points (the walks end at the first
    point r below or at the window's sentinel, no stored count; the skip counts at their caps),
    bit-exact."""
    monkeypatch.setenv("PCP_TERRAIN_BLOCKS", "2")
    monkeypatch.setenv("PCP_FINE_SKIP", skip)
    rng = np.random.default_rng(5)
    n = 70_000
    cube = np.column_stack([rng.uniform(1.0, 1.05, n), rng.uniform(0.0, 0.05, n),
                            rng.uniform(0.0, 0.05, n)])
    cloud = np.zeros((n, 8), np.float32)
    cloud[:, :3] = cube
    poses = np.array([[0.0, 0.0, 0.3, -0.2, 0.0]])
    fan = _abi.fan_params(n_az=64, n_el=8, el_min_deg=-30.0, el_max_deg=10.0, max_distance=3.0)
    with _abi.Context(0) as ctx:
        ctx.set_terrain(cloud, point_step=32)
        blocked, units, fh, _ = ctx.raycast_fan(poses, fan, want_first_hit=True)
        assert ctx.terrain_info()["scan_layout"] == "fine"
        r_blocked, r_units, r_fh = oracle.raycast_fan(oracle.Cloud(cloud), poses, 64, 8,
                                                      fan.el_min, fan.el_max, 3.0)
        np.testing.assert_array_equal(fh, r_fh)
        np.testing.assert_array_equal(blocked, r_blocked)
        np.testing.assert_array_equal(units, r_units)
        assert blocked[0] > 0


# ---------------------------------------------------------------------------------- multi-GPU
_DEVICE_KEYS_CHECK = r"""
import sys
import numpy as np
import torch
torch.cuda.init()                      # torch's HIP runtime first, as in bench.py
sys.path.insert(0, sys.argv[1])
import bench
from pointcloud_processor_amd import _abi, synth
from pointcloud_processor_amd import dist as pd
scene = synth.terrain_scene()
gpu = _abi.Context(0)
gpu.set_terrain(scene.terrain, point_step=32)
poses, _ = bench._poses_for(gpu, bench._grid_bbox(scene.area), scene.zx120_pose5, 96)
fan = _abi.fan_params(n_az=256, n_el=64)
b1, u1, _, _ = gpu.raycast_fan(poses, fan)
P, world = poses.shape[0], 4
ref_keys, ref_best = pd.reduce_fan(b1, 0, P, P)
dev = torch.device("cuda", 0)
units = torch.zeros(P, dtype=torch.int64, device=dev)
red = None
for r in range(world):
    lo, hi = pd.shard(P, world, r)
    k = torch.empty(P, dtype=torch.int64, device=dev)
    # no stream handle: torch's runtime is not libpcp's (the call returns with the keys written)
    gpu.raycast_fan_keys(np.ascontiguousarray(poses[lo:hi]), fan, lo, P, k.data_ptr(),
                         units.data_ptr() + 8 * lo, None)
    red = k if red is None else torch.minimum(red, k)
kh = red.cpu().numpy()
assert np.array_equal(kh >> 32, ref_keys)
assert np.array_equal(kh & 0xFFFFFFFF, np.arange(P))
assert int(kh.min()) & 0xFFFFFFFF == ref_best
assert np.array_equal(units.cpu().numpy().astype(np.uint64), u1)
k = torch.zeros(P, dtype=torch.int64, device=dev)
gpu.raycast_fan_keys(poses[:0].copy(), fan, P, P, k.data_ptr(), None, None)
assert bool((k == np.iinfo(np.int64).max).all())
print("device keys ok", P, ref_best)
"""


def test_fan_device_keys_match_reduce_fan():
    """bench.py --gpus N over RCCL: pcp_raycast_fan_keys writes each rank's keys into a torch
    device vector (no host copy), the collective is an int64 MIN.  Four ranks' shards on one
    device, their vectors combined by torch.minimum (the all-reduce's arithmetic): blocked
    counts, units and the argmin bit-identical to the host path (raycast_fan ->
    dist.reduce_fan).  In its own process, torch's HIP runtime initialised first as in
    bench.py (torch bundles its own ROCm runtime beside the one libpcp links)."""
    import subprocess
    import sys
    from pathlib import Path

    root = str(Path(__file__).resolve().parents[1])
    r = subprocess.run([sys.executable, "-c", _DEVICE_KEYS_CHECK, root], capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "device keys ok" in r.stdout


def test_fan_allreduce_own_communicator(gpu, loaded, scene):
    """bench.py --gpus N with libpcp's OWN RCCL communicator (one HIP runtime in the process):
    pcp_comm_init_rank over one rank, then pcp_raycast_fan_allreduce -- keys on the context's
    device vector, ncclAllReduce(MIN) on its stream, the reduced vector back once -- bit-identical
    to the host path (raycast_fan -> dist.reduce_fan): every blocked count, the units, the argmin.
    A shard that leaves poses unwritten is refused (PCP_E_STATE), an empty shard is not."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import bench
    from pointcloud_processor_amd import dist as pd

    poses, _ = bench._poses_for(gpu, bench._grid_bbox(scene.area), scene.zx120_pose5, 96)
    fan = _abi.fan_params(n_az=256, n_el=64)
    b1, u1, _, _ = gpu.raycast_fan(poses, fan)
    P = poses.shape[0]
    ref_keys, ref_best = pd.reduce_fan(b1, 0, P, P)
    with _abi.Context(0) as ctx:
        assert ctx.comm_info() == (0, 0)
        with pytest.raises(_abi.PcpError):          # no communicator yet
            ctx.raycast_fan_allreduce(poses, fan, 0, P)
        ctx.comm_init_rank(1, _abi.comm_unique_id(), 0)
        assert ctx.comm_info() == (1, 0)
        ctx.set_terrain(scene.terrain, point_step=32)
        for rep in range(3):                         # steady state: same answer every query
            blocked = np.zeros(P, np.uint32)
            units = np.zeros(P, np.uint64)
            best, ms = ctx.raycast_fan_allreduce(poses, fan, 0, P, blocked, units, timed=rep == 2)
            np.testing.assert_array_equal(blocked, ref_keys)
            np.testing.assert_array_equal(units, u1)
            assert best == ref_best == int(np.argmin(b1))
        assert ms is not None and ms >= 0.0
        with pytest.raises(_abi.PcpError):           # poses [P/2, P) written by no rank
            ctx.raycast_fan_allreduce(np.ascontiguousarray(poses[:P // 2]), fan, 0, P)
        best, _ = ctx.raycast_fan_allreduce(poses[:0].copy(), fan, 0, 0)
        assert best == -1


def test_score_allreduce_own_communicator(oracle, loaded, scene, cells, aux):
    """runOptimization's scoring for N processes in ONE RCCL collective
    (pcp_score_poses_allreduce: [P totals | P covered | 3 x C newest-pose flag keys | health],
    ncclAllReduce(MAX) on the context's stream).  At N = 1 it is bit-identical to
    pcp_score_poses on the same context: every total's bits, the covered counts, the stale flags
    of two ticks (the second from the first's flags, poses reversed), the report; the oracle
    agrees on the flags and the best index.  A rank whose arguments fail before the collective
    still runs it with a poisoned health word: it reports its own error, and the communicator
    stays usable (the next query is exact again); poses that no rank scored are reported."""
    T, A = loaded
    params = _abi.default_vl_params()
    zx = np.ascontiguousarray(scene.zx120_pose5, np.float64)
    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.set_aux_cloud(aux, point_step=32)
        ctx.set_cells(cells.xyz, cells.normals)
        poses = ctx.generate_candidates(cells.grid_bbox, params, scene.zx120_pose5)
        P, C = poses.shape[0], cells.xyz.shape[0]
        rep = _abi.VlReport()
        fl = np.zeros(C, np.uint8)
        with pytest.raises(_abi.PcpError):          # no communicator yet
            ctx.score_poses_allreduce(poses, zx, params, 0, P, fl, None, None, rep)
        ctx.comm_init_rank(1, _abi.comm_unique_id(), 0)
        f1, f2, fr = np.zeros(C, np.uint8), np.zeros(C, np.uint8), np.zeros(C, np.uint8)
        for tick, pz in enumerate((poses, poses[::-1].copy())):
            t1, c1, r1 = ctx.score_poses(pz, zx, params, f1)
            t2, c2 = np.zeros(P, np.float64), np.zeros(P, np.int32)
            rep2 = _abi.VlReport()
            ms = ctx.score_poses_allreduce(pz, zx, params, 0, P, f2, t2, c2, rep2, timed=True)
            assert ms is not None and ms >= 0.0
            np.testing.assert_array_equal(t2.view(np.uint64), t1.view(np.uint64))
            np.testing.assert_array_equal(c2, c1)
            np.testing.assert_array_equal(f2, f1)
            assert rep2.as_dict() == r1.as_dict(), tick
            _, _, rr = oracle.score_poses(T, A, cells.xyz, cells.normals, pz, scene.zx120_pose5,
                                          oracle.vl_params(), fr)
            np.testing.assert_array_equal(f2, fr)
            assert rep2.best_idx == rr.best_idx
        # a bad shard fails on this rank only; the collective still ran (health word poisoned)
        with pytest.raises(_abi.PcpError):
            ctx.score_poses_allreduce(poses, zx, params, 5, P, f2.copy(), None, None, rep)
        assert ctx.comm_info() == (1, 0)
        f3 = np.zeros(C, np.uint8)
        t3 = np.zeros(P, np.float64)
        ctx.score_poses_allreduce(poses, zx, params, 0, P, f3, t3, None, rep)
        t4, _, r4 = ctx.score_poses(poses, zx, params, np.zeros(C, np.uint8))
        np.testing.assert_array_equal(t3.view(np.uint64), t4.view(np.uint64))
        assert rep.best_idx == r4.best_idx
        # poses no rank scored (here: [0, 3) of a one-rank communicator) are an error, as the
        # fan's unwritten keys are -- not zero totals; the caller's flags stay as they were
        f5 = np.full(C, 0x5A, np.uint8)
        with pytest.raises(_abi.PcpError, match="scored by no rank"):
            ctx.score_poses_allreduce(poses[3:], zx, params, 3, P, f5, None, None, rep)
        assert (f5 == 0x5A).all()
        ctx.score_poses_allreduce(poses, zx, params, 0, P, f3 * 0, t3, None, rep)
        np.testing.assert_array_equal(t3.view(np.uint64), t4.view(np.uint64))
        # the fan's collective carries the same health word: a bad shard, then an exact query
        fan = _abi.fan_params(n_az=128, n_el=32)
        with pytest.raises(_abi.PcpError):
            ctx.raycast_fan_allreduce(poses, fan, 3, P)
        bl = np.zeros(P, np.uint32)
        best, _ = ctx.raycast_fan_allreduce(poses, fan, 0, P, bl)
        b_ref, _, _, best_ref = ctx.raycast_fan(poses, fan)
        np.testing.assert_array_equal(bl, b_ref[:P])
        assert best == best_ref


@pytest.mark.parametrize("onepass", ["1", "0"])
def test_exclusive_scan_tile_boundaries(onepass, monkeypatch):
    """the index builds' device scan on its own.  Back-to-back scans sized to 1, 2,
    63, 64 (the one-pass look-back's largest) and 65 (three launches) tiles of 2,048, growing
    and shrinking (the look-back state regrows, the epoch and ticket advance), each equal to
    numpy's, with PCP_SCAN_ONEPASS=1 (default) and 0."""
    monkeypatch.setenv("PCP_SCAN_ONEPASS", onepass)
    rng = np.random.default_rng(11)
    with _abi.Context(0) as ctx:
        for tiles in (1, 2, 63, 64, 65, 2, 64, 3, 200, 64, 1):
            for n in (tiles * 2048, tiles * 2048 - 5):
                if n <= 0:
                    continue
                a = rng.integers(0, 1000, n, dtype=np.uint32)
                ref = np.zeros(n + 1, np.uint64)
                ref[1:] = np.cumsum(a, dtype=np.uint64)
                got = ctx.debug_exclusive_scan(a)
                np.testing.assert_array_equal(got, ref.astype(np.uint32)), (tiles, n)


def _cell_census(got_sm, got_sz, ref_sm, ref_sz):
    """Per-cell comparison of evaluateCellScore values: cells whose score differs, by how many
    ulps, and the signed balance of the differences (a systematic drift leans one way)."""
    g = np.concatenate([got_sm.ravel(), got_sz])
    r = np.concatenate([ref_sm.ravel(), ref_sz])
    d = parity.ulps(g, r)
    pos = r > 0
    up = int(((g > r) & (d > 0)).sum())
    return {"cells": int(g.size), "positive": int(pos.sum()), "differ": int((d > 0).sum()),
            "up": up, "down": int((d > 0).sum()) - up, "max_ulps": float(d.max(initial=0)),
            "zero_mismatch": int(((g > 0) != pos).sum())}


def test_parity_bar_per_cell(oracle, loaded, scene, cells, aux):
    """VERDICT r5 item 5, at the cells: evaluateCellScore per (pose, cell) on the device
    (pcp_score_matrix) against the oracle's (orc_score_matrix) on the 91-candidate tick.  The
    production build rounds acos / sin correctly (pcp_crmath.h), as glibc does but for its rare
    near ties: 0.16 % of the positive cell scores differ, by 1-4 ulps (ocml's own functions
    left 9 %, up to 8 ulps); the `make perturb` (every cell) and `make perturb8` (every 8th cell)
    builds fail the per-cell bar (tests/parity.py: cell_bar)."""
    T, A = loaded
    params = _abi.default_vl_params()
    zx = np.ascontiguousarray(scene.zx120_pose5, np.float64)
    res = {}
    for tag, path in (("prod", None), ("perturbed", str(PERTURB_LIB)),
                      ("perturbed8", str(PERTURB8_LIB))):
        with _abi.Context(0, lib_path=path) as ctx:
            ctx.set_terrain(scene.terrain, point_step=32)
            ctx.set_aux_cloud(aux, point_step=32)
            ctx.set_cells(cells.xyz, cells.normals)
            poses = ctx.generate_candidates(cells.grid_bbox, params, scene.zx120_pose5)
            sm_sz = ctx.score_matrix(poses, zx, params)
            tot, _, _ = ctx.score_poses(poses, zx, params, np.zeros(cells.xyz.shape[0], np.uint8))
            res[tag] = (poses, sm_sz, tot)
    poses = res["prod"][0]
    r_sm, r_sz = oracle.score_matrix(T, A, cells.xyz, cells.normals, poses, scene.zx120_pose5,
                                     oracle.vl_params())
    r_tot, _ = oracle.score_totals(T, A, cells.xyz, cells.normals, poses, scene.zx120_pose5,
                                   oracle.vl_params())
    for tag in res:
        np.testing.assert_array_equal(res[tag][0], poses)
        cen = _cell_census(*res[tag][1], r_sm, r_sz)
        print("cell census", tag, cen, parity.cell_bar(cen), "totals",
              parity.totals_report(res[tag][2], r_tot))
        assert cen["zero_mismatch"] == 0
        assert parity.cell_bar(cen) == (tag == "prod"), (tag, cen)
        # the same tick's totals under the exact bar: the cells that differ (glibc's near ties)
        # do not reach a total's bits, either drift does
        assert parity.totals_exact(res[tag][2], r_tot) == (tag == "prod"), tag


def test_score_stats_and_burst(loaded, scene, cells, aux):
    """The reference-mode roofline's inputs: pcp_score_poses_stats counts
    the visibility rays' gather lane-loads with a twin of k_score_cells -- deterministic, every
    walk start follows a probe, the fine-window copy needs no directory loads -- and
    pcp_score_poses_burst times the production launch; neither touches the caller's flags nor
    changes the next query's results."""
    params = _abi.default_vl_params()
    zx = np.ascontiguousarray(scene.zx120_pose5, np.float64)
    with _abi.Context(0) as ctx:
        ctx.set_terrain(scene.terrain, point_step=32)
        ctx.set_aux_cloud(aux, point_step=32)
        ctx.set_cells(cells.xyz, cells.normals)
        poses = ctx.generate_candidates(cells.grid_bbox, params, scene.zx120_pose5)
        C = cells.xyz.shape[0]
        t0, c0, r0 = ctx.score_poses(poses, zx, params, np.zeros(C, np.uint8))
        st = ctx.score_poses_stats(poses, zx, params)
        assert st == ctx.score_poses_stats(poses, zx, params)
        assert st["probes"] >= st["walk_starts"] > 0 and st["point_tests"] > 0
        assert st["directory_loads"] == 0
        # more poses, more rays: the counts grow
        st2 = ctx.score_poses_stats(np.concatenate([poses, poses]), zx, params)
        assert st2["probes"] > st["probes"]
        ms = ctx.score_poses_burst(poses, zx, params, reps=5)
        assert ms > 0.0
        t1, c1, r1 = ctx.score_poses(poses, zx, params, np.zeros(C, np.uint8))
        np.testing.assert_array_equal(t1.view(np.uint64), t0.view(np.uint64))
        np.testing.assert_array_equal(c1, c0)
        assert r1.as_dict() == r0.as_dict()


def test_fan_keys_wait_stream_then_fan(gpu, loaded, scene, oracle):
    """a keys query handed to a libpcp wait_stream returns before its pose upload
    has read the pinned staging; the next fan query on the context (other poses) must not
    overwrite that staging first.  Keys of the first query == the oracle's blocked counts of its
    poses, the second query's counts == its own."""
    fan = _abi.fan_params(n_az=128, n_el=32)
    sc = scene
    rng = np.random.default_rng(7)
    a = np.column_stack([rng.uniform(-5, 5, 48), rng.uniform(-5, 5, 48), rng.uniform(0.5, 2.0, 48),
                         rng.uniform(-0.6, 0.0, 48), rng.uniform(-3, 3, 48)])
    b = a.copy()
    b[:, 4] += 1.0
    b[:, 2] += 0.7
    T = oracle.Cloud(sc.terrain)
    ra, _, _ = oracle.raycast_fan(T, a, 128, 32, fan.el_min, fan.el_max, fan.max_distance,
                                  want_first_hit=False)
    rb, _, _ = oracle.raycast_fan(T, b, 128, 32, fan.el_min, fan.el_max, fan.max_distance,
                                  want_first_hit=False)
    assert not np.array_equal(ra, rb)
    with _abi.Context(0) as ctx:
        ctx.set_terrain(sc.terrain, point_step=32)
        st = ctx.stream_create()
        try:
            keys = ctx.dev_alloc(8 * a.shape[0])
            for _ in range(3):
                ctx.raycast_fan_keys(np.ascontiguousarray(a), fan, 0, a.shape[0], keys, None, st)
                got_b, _, _, _ = ctx.raycast_fan(b, fan)      # rewrites the pinned pose staging
                kh = np.zeros(a.shape[0], np.int64)
                ctx.synchronize()
                ctx.d2h(kh, keys)
                np.testing.assert_array_equal((kh >> 32).astype(np.uint32), ra)
                np.testing.assert_array_equal(got_b, rb)
            ctx.dev_free(keys)
        finally:
            ctx.stream_destroy(st)


# ------------------------------------------------- long range: step tables up to and past LDS
# max_distance -> the step table's length K: 77.3 is the last table the kernels read from LDS
# (kStepLds = 256), 77.6 the first they read from global memory (the <false> instantiations of
# k_score_cells / _wide / _stats and the fan's fall-back from the XCD-chunked kernels), 110.0 a
# LiDAR's real range.
LONG_K = {77.3: 256, 77.6: 257, 110.0: 365}
LONG_MD = tuple(LONG_K)
LONG_EL_DEG = 6.0
# (PCP_TERRAIN_BLOCKS, PCP_TERRAIN_FINE, PCP_FINE_TILE, layout) of LAYOUTS below: the fine
# windows with FN 4 / 1 / 8 records, 2 x 2 x 2 blocks, per-cell runs
LONG_LAYOUTS = [("2", "2", "1", "fine"), ("2", "2", "0", "fine"), ("2", "2", "2", "fine"),
                ("2", "3", "2", "fine"), ("2", "0", "1", "blocks"), ("0", "3", "1", "cells")]


def _long_range_scene(seed=5):
    """A 112 m corridor, 150 k points of 16 bytes: a thin ground slab over x in [-2, 110],
    y in [-8, 8]; 0.3 m wall slabs at x = 60 (y < -3), x = 85 (0 < y < 3) and x = 104 (full
    width); one slab over x in [76.9, 77.5] (-3 < y < 0), which the samples k = 255 (77.0 m) and
    k = 256 (77.3 m) of the near poses' rays fall into.  Eight fan poses: seven near x = 0 at
    various y, z, pitch and yaw, one at the far end facing back.  600 scoring cells float over
    x in [70, 103] (behind the walls or in the gaps between them); the scoring poses are three
    of the near ones, the far one and one among the cells (in range at max_distance 15 too)."""
    from types import SimpleNamespace

    rng = np.random.default_rng(seed)

    def slab(n, x0, x1, y0, y1, z0, z1):
        return rng.uniform([x0, y0, z0], [x1, y1, z1], (n, 3))

    parts = [slab(84_000, -2.0, 110.0, -8.0, 8.0, -0.02, 0.02),
             slab(12_000, 59.85, 60.15, -8.0, -3.0, 0.0, 3.2),
             slab(9_000, 76.9, 77.5, -3.0, 0.0, 0.0, 3.2),
             slab(8_000, 84.85, 85.15, 0.0, 3.0, 0.0, 3.2),
             slab(37_000, 103.85, 104.15, -8.0, 8.0, 0.0, 4.0)]
    cloud = np.zeros((sum(p.shape[0] for p in parts), 4), np.float32)
    cloud[:, :3] = np.concatenate(parts)
    cloud = np.ascontiguousarray(cloud[rng.permutation(cloud.shape[0])])
    near = np.array([[0.0, 0.0, 1.5, 0.0, 0.0], [-0.4, -1.7, 2.0, -0.01, 0.02],
                     [0.3, 1.1, 1.2, 0.01, -0.03], [0.13, -5.5, 2.4, 0.0, 0.05],
                     [-1.0, 4.5, 1.8, 0.005, -0.04], [0.45, -0.9, 1.0, 0.015, 0.0],
                     [-0.2, 6.0, 2.2, -0.005, -0.06]])
    far = np.array([[108.0, 0.5, 1.6, 0.0, np.pi]])
    mid = np.array([[86.0, 5.0, 1.6, 0.0, np.pi]])
    xyz = rng.uniform([70.0, -8.0, 0.5], [103.0, 8.0, 3.0], (600, 3))
    nrm = rng.normal(size=(600, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    many = np.column_stack([rng.uniform(-1.0, 1.0, 60), rng.uniform(-7.0, 7.0, 60),
                            rng.uniform(1.0, 2.5, 60), rng.uniform(-0.02, 0.02, 60),
                            rng.uniform(-0.06, 0.06, 60)])
    return SimpleNamespace(cloud=cloud, fan_poses=np.concatenate([near, far]),
                           score_poses=np.concatenate([near[:3], far, mid]), n_near=3,
                           many_poses=many, xyz=xyz, nrm=nrm,
                           zx=np.array([1.0, 2.0, 1.4, 0.0, 0.0]),
                           # (its centre below the sensor height: the candidates look slightly
                           # up from straight down, so the cells 30-100 m away are in their FOV)
                           cand_bbox=np.array([-4.0, 40.0, -8.0, 8.0, -3.0, 1.0]))


@pytest.fixture(scope="module")
def long_range(oracle):
    """The long-range scene, its oracle tree and a cache of the oracle's results: every
    reference is computed once, shared by the tests below and never written to."""
    lr = _long_range_scene()
    lr.T = oracle.Cloud(lr.cloud)
    lr.ref = {}
    return lr


def _long_fan_ref(oracle, lr, md, n_az, n_el):
    """(blocked, units, first hits) of the oracle for the scene's eight fan poses."""
    key = ("fan", md, n_az, n_el)
    if key not in lr.ref:
        el = math.radians(LONG_EL_DEG)
        r = oracle.raycast_fan(lr.T, lr.fan_poses, n_az, n_el, -el, el, md)
        for a in r:
            a.setflags(write=False)
        lr.ref[key] = r
    return lr.ref[key]


def _long_score_ref(oracle, lr, md, poses_name="score_poses"):
    """The oracle's scoring of the scene at max_distance md: two ticks whose flags carry over
    (the second with the poses reversed), the per-cell matrix with and without the terrain."""
    key = ("score", md, poses_name)
    if key not in lr.ref:
        poses = getattr(lr, poses_name)
        p = oracle.vl_params(max_distance=md)
        fl = np.zeros(lr.xyz.shape[0], np.uint8)
        ticks = []
        oracle.set_threads(8)
        try:
            for ps in (poses, poses[::-1].copy()):
                tot, cov, rep = oracle.score_poses(lr.T, None, lr.xyz, lr.nrm, ps, lr.zx, p, fl)
                ticks.append((tot, cov, rep.as_dict(), fl.copy()))
            sm, sz = oracle.score_matrix(lr.T, None, lr.xyz, lr.nrm, poses, lr.zx, p)
            sm0, _ = oracle.score_matrix(None, None, lr.xyz, lr.nrm, poses, lr.zx, p)
        finally:
            oracle.set_threads(1)
        for a in (sm, sz, sm0) + tuple(x for t in ticks for x in (t[0], t[1], t[3])):
            a.setflags(write=False)
        lr.ref[key] = {"ticks": ticks, "sm": sm, "sz": sz, "sm0": sm0}
    return lr.ref[key]


def _long_fan_params(n_az, n_el, md):
    return _abi.fan_params(n_az=n_az, n_el=n_el, el_min_deg=-LONG_EL_DEG, el_max_deg=LONG_EL_DEG,
                           max_distance=md)


def _set_layout_env(monkeypatch, mode, fine, tile):
    monkeypatch.setenv("PCP_TERRAIN_BLOCKS", mode)
    monkeypatch.setenv("PCP_TERRAIN_FINE", fine)
    monkeypatch.setenv("PCP_FINE_TILE", tile)
    monkeypatch.setenv("PCP_FINE_PACK", "1")


def _assert_report_equal(got: dict, ref: dict, exact_totals=True):
    for k in got:
        if k in ("best_score", "zx120_total_score"):
            parity.assert_totals(got[k], ref[k])
            if exact_totals:
                parity.assert_totals_exact(got[k], ref[k])
        else:
            assert got[k] == ref[k], k


@pytest.mark.parametrize("n_az,n_el", [(1024, 8), (100, 37)])
@pytest.mark.parametrize("md", LONG_MD)
def test_long_range_fan(oracle, long_range, md, n_az, n_el, monkeypatch):
    """The ray fan at max_distance 77.3 / 77.6 / 110 (K = 256: the last step table in LDS, 257:
    the first in global memory, 365) on the long-range scene: first hits, blocked counts and
    units equal the oracle's exactly, for 8 poses (P % 8 == 0: the XCD-chunked kernels at
    K = 256, their K > kStepLds fall-back to the plain launch from K = 257) and for 3 poses, on
    the fine-window (FN 4 / 1 / 8), block and per-cell layouts; 1024 x 8 is the uniform-ring
    fan, 100 x 37 has rings spanning waves and a ragged last wave.  The oracle's output first
    shows that the path is exercised (hits at k >= 256, at exactly k = 255 / 256, misses).  At
    K = 365 the stats twin and the burst launch run once as well: deterministic counts, a
    positive time, the next query's results unchanged bit for bit."""
    lr = long_range
    K = LONG_K[md]
    assert _abi.step_table(md - 0.08).size == K
    assert (K <= 256) == (md == 77.3)
    fan = _long_fan_params(n_az, n_el, md)
    r_blocked, r_units, r_fh = _long_fan_ref(oracle, lr, md, n_az, n_el)
    # reference-only preconditions
    assert (r_fh == -1).any() and ((r_fh >= 0) & (r_fh < 256)).any()
    if md == 110.0:
        assert int((r_fh >= 256).sum()) >= 50 and r_fh.max() > 300
    elif md == 77.6:
        assert (r_fh == 256).any() and r_fh.max() == 256
    else:
        assert r_fh.max() == 255
    three = [0, 3, 7]
    for mode, fine, tile, layout in LONG_LAYOUTS:
        _set_layout_env(monkeypatch, mode, fine, tile)
        with _abi.Context(0) as ctx:
            ctx.set_terrain(lr.cloud, point_step=16)
            blocked, units, fh, best = ctx.raycast_fan(lr.fan_poses, fan, want_first_hit=True)
            b3, u3, fh3, best3 = ctx.raycast_fan(lr.fan_poses[three], fan, want_first_hit=True)
            assert ctx.terrain_info()["scan_layout"] == layout
        tag = (mode, fine, tile)
        bad = int(np.count_nonzero(fh != r_fh))
        assert bad == 0, (tag, f"{bad} of {fh.size} first hits differ")
        np.testing.assert_array_equal(blocked, r_blocked, err_msg=str(tag))
        np.testing.assert_array_equal(units, r_units, err_msg=str(tag))
        assert best == int(np.argmin(r_blocked)), tag
        np.testing.assert_array_equal(fh3, r_fh[three], err_msg=str(tag))
        np.testing.assert_array_equal(b3, r_blocked[three], err_msg=str(tag))
        np.testing.assert_array_equal(u3, r_units[three], err_msg=str(tag))
        assert best3 == int(np.argmin(r_blocked[three])), tag
    if md != 110.0:
        return
    for name in ("PCP_TERRAIN_BLOCKS", "PCP_TERRAIN_FINE", "PCP_FINE_TILE", "PCP_FINE_PACK"):
        monkeypatch.delenv(name)
    with _abi.Context(0) as ctx:   # the defaults
        ctx.set_terrain(lr.cloud, point_step=16)
        b0, u0, fh0, _ = ctx.raycast_fan(lr.fan_poses, fan, want_first_hit=True)
        np.testing.assert_array_equal(fh0, r_fh)
        st = ctx.raycast_fan_stats(lr.fan_poses, fan)
        assert st == ctx.raycast_fan_stats(lr.fan_poses, fan)
        assert st["samples_visited"] >= st["scanned_stencils"] > 0 and st["point_tests"] > 0
        assert ctx.raycast_fan_burst(lr.fan_poses, fan, reps=3) > 0.0
        b1, u1, fh1, _ = ctx.raycast_fan(lr.fan_poses, fan, want_first_hit=True)
        np.testing.assert_array_equal(fh1, fh0)
        np.testing.assert_array_equal(b1, b0)
        np.testing.assert_array_equal(u1, u0)
        np.testing.assert_array_equal(b1, r_blocked)
        np.testing.assert_array_equal(u1, r_units)


def _long_score_preconditions(lr, ref, md):
    """Reference-only: at 110 m every near pose sees, past 77.5 m (k >= 256), at least 100
    cells and has at least 100 more hidden by the terrain alone."""
    if md != 110.0:
        return
    poses = lr.score_poses[:lr.n_near]
    d = np.linalg.norm(lr.xyz[None, :, :] - poses[:, None, :3], axis=2)
    far = d > 77.5
    vis = ((ref["sm"][:lr.n_near] > 0) & far).sum(1)
    blk = ((ref["sm0"][:lr.n_near] > 0) & (ref["sm"][:lr.n_near] == 0) & far).sum(1)
    assert vis.min() >= 100 and blk.min() >= 100, (vis, blk)


def _long_score_check(ctx, lr, ref, md, poses, exact_totals=True, tag=""):
    """Two ticks whose flags carry over and the per-cell matrix against the cached oracle
    results: flags, covered counts, best index and report counters exact, totals under the
    bars of tests/parity.py, cells under cell_bar with no zero / positive mismatch."""
    params = _abi.default_vl_params(max_distance=md)
    fg = np.zeros(lr.xyz.shape[0], np.uint8)
    for t, ps in enumerate((poses, poses[::-1].copy())):
        r_tot, r_cov, r_rep, r_fl = ref["ticks"][t]
        tot, cov, rep = ctx.score_poses(ps, lr.zx, params, fg)
        print("long range", tag, "md", md, "tick", t, "totals", parity.totals_report(tot, r_tot))
        np.testing.assert_array_equal(fg, r_fl)
        np.testing.assert_array_equal(cov, r_cov)
        parity.assert_totals(tot, r_tot)
        if exact_totals:
            parity.assert_totals_exact(tot, r_tot)
        _assert_report_equal(rep.as_dict(), r_rep, exact_totals)
    srt = np.sort(ref["ticks"][0][0])[::-1]
    assert (srt[0] - srt[1]) > 1e-9 * srt[0]     # the argmax is decidable
    sm, sz = ctx.score_matrix(poses, lr.zx, params)
    cen = _cell_census(sm, sz, ref["sm"], ref["sz"])
    print("long range", tag, "md", md, "cell census", cen)
    assert cen["zero_mismatch"] == 0, cen
    assert parity.cell_bar(cen), cen
    return cen


@pytest.mark.parametrize("wide", ["1", "0"])
@pytest.mark.parametrize("md", LONG_MD)
def test_long_range_score(oracle, long_range, md, wide, monkeypatch):
    """Reference-mode scoring at K = 256 / 257 / 365 on the long-range scene, 600 cells x 6
    rows: k_score_cells_wide<SL, 16> (the default for so few rays) and, with PCP_SCORE_WIDE=0,
    k_score_cells<SL> -- SL false from K = 257.  Flags, covered counts, best index and report
    counters exact over two ticks; no cell positive on one side only; cells under cell_bar;
    totals bit-identical to the oracle's: the first run on an MI355X showed 0 differing totals
    in every case (both ticks, and the 12 candidates' of pcp_generate_and_score), so all are
    held to the exact bar.  Cells differing there, one ulp each, the same with either kernel:
    1 of 1,018 positive ones at K = 256, 2 of 1,031 at K = 257, 7 of 1,996 at K = 365.
    At K = 365 the stats twin (k_score_cells_stats<false>) runs too, and
    pcp_generate_and_score is compared with the two calls and with the oracle's candidates."""
    lr = long_range
    assert _abi.step_table(md - 0.08).size == LONG_K[md]
    ref = _long_score_ref(oracle, lr, md)
    _long_score_preconditions(lr, ref, md)
    monkeypatch.setenv("PCP_SCORE_WIDE", wide)
    poses = lr.score_poses
    assert (poses.shape[0] + 1) * lr.xyz.shape[0] <= 1 << 15   # the wide kernel's range
    params = _abi.default_vl_params(max_distance=md)
    with _abi.Context(0) as ctx:
        ctx.set_terrain(lr.cloud, point_step=16)
        ctx.set_cells(lr.xyz, lr.nrm)
        _long_score_check(ctx, lr, ref, md, poses, tag=f"wide={wide}")
        if md != 110.0:
            return
        C = lr.xyz.shape[0]
        t0, c0, r0 = ctx.score_poses(poses, lr.zx, params, np.zeros(C, np.uint8))
        st = ctx.score_poses_stats(poses, lr.zx, params)
        assert st == ctx.score_poses_stats(poses, lr.zx, params)
        assert st["probes"] >= st["walk_starts"] > 0 and st["point_tests"] > 0
        assert st["directory_loads"] == 0
        st2 = ctx.score_poses_stats(np.concatenate([poses, poses]), lr.zx, params)
        assert st2["probes"] > st["probes"]
        assert ctx.score_poses_burst(poses, lr.zx, params, reps=3) > 0.0
        t1, c1, r1 = ctx.score_poses(poses, lr.zx, params, np.zeros(C, np.uint8))
        np.testing.assert_array_equal(t1.view(np.uint64), t0.view(np.uint64))
        np.testing.assert_array_equal(c1, c0)
        assert r1.as_dict() == r0.as_dict()
        # one round trip against the two calls, and both against the oracle
        gp = _abi.default_vl_params(max_distance=md, num_candidates=16)
        op = oracle.vl_params(max_distance=md, num_candidates=16)
        fa, fb, fr = (np.zeros(C, np.uint8) for _ in range(3))
        cand = ctx.generate_candidates(lr.cand_bbox, gp, lr.zx)
        tot, cov, rep = ctx.score_poses(cand, lr.zx, gp, fa)
        p2, tot2, cov2, rep2 = ctx.generate_and_score(lr.cand_bbox, gp, lr.zx, fb)
        np.testing.assert_array_equal(p2, cand)
        np.testing.assert_array_equal(tot2.view(np.uint64), tot.view(np.uint64))
        np.testing.assert_array_equal(cov2, cov)
        np.testing.assert_array_equal(fb, fa)
        assert rep2.as_dict() == rep.as_dict()
        r_cand = oracle.generate_candidates(lr.T, lr.cand_bbox, op, lr.zx)
        assert cand.shape == r_cand.shape and cand.shape[0] >= 8
        np.testing.assert_array_equal(cand[:, :3], r_cand[:, :3])
        parity.assert_angles(cand[:, 3:], r_cand[:, 3:])
        r_tot, r_cov, r_rep = oracle.score_poses(lr.T, None, lr.xyz, lr.nrm, cand, lr.zx, op, fr)
        print("long range generate_and_score totals", parity.totals_report(tot2, r_tot))
        np.testing.assert_array_equal(fb, fr)
        np.testing.assert_array_equal(cov2, r_cov)
        parity.assert_totals_exact(tot2, r_tot)
        assert rep2.best_idx == r_rep.best_idx and r_cov.max() > 100


def test_long_range_score_many_poses(oracle, long_range):
    """60 poses x 600 cells (61 rows: past kWideMaxRays) with no knob set: the production choice
    at max_distance 110 is k_score_cells<false>, one lane per ray, the step table in global
    memory.  Same assertions as test_long_range_score, the totals under the exact bar (first
    MI355X run: 0 of 60 totals differ on either tick; 47 of 20,436 positive cells do, 26 up and
    21 down, the largest by 8 ulps)."""
    lr = long_range
    md = 110.0
    assert (lr.many_poses.shape[0] + 1) * lr.xyz.shape[0] > 1 << 15
    ref = _long_score_ref(oracle, lr, md, "many_poses")
    with _abi.Context(0) as ctx:
        ctx.set_terrain(lr.cloud, point_step=16)
        ctx.set_cells(lr.xyz, lr.nrm)
        _long_score_check(ctx, lr, ref, md, lr.many_poses, tag="60 poses")


def test_long_range_step_table_cache(oracle, long_range):
    """ensure_steps caches the step table by its end, shares the device buffer between the fan
    and the scoring and regrows it: on ONE context, queries at max_distance 15 -> 110 -> 15 ->
    77.6 -> 110, fan and scoring taking turns at being the first to ask for a new table, each
    compared with the oracle -- a stale or short table shows as wrong first hits or flags."""
    lr = long_range
    n_az, n_el = 100, 37

    def fan_q(ctx, md):
        r_blocked, r_units, r_fh = _long_fan_ref(oracle, lr, md, n_az, n_el)
        blocked, units, fh, _ = ctx.raycast_fan(lr.fan_poses, _long_fan_params(n_az, n_el, md),
                                                want_first_hit=True)
        np.testing.assert_array_equal(fh, r_fh, err_msg=f"fan {md}")
        np.testing.assert_array_equal(blocked, r_blocked, err_msg=f"fan {md}")
        np.testing.assert_array_equal(units, r_units, err_msg=f"fan {md}")

    def score_q(ctx, md):
        r_tot, r_cov, r_rep, r_fl = _long_score_ref(oracle, lr, md)["ticks"][0]
        fg = np.zeros(lr.xyz.shape[0], np.uint8)
        tot, cov, rep = ctx.score_poses(lr.score_poses, lr.zx,
                                        _abi.default_vl_params(max_distance=md), fg)
        np.testing.assert_array_equal(fg, r_fl, err_msg=f"score {md}")
        np.testing.assert_array_equal(cov, r_cov, err_msg=f"score {md}")
        parity.assert_totals_exact(tot, r_tot)
        _assert_report_equal(rep.as_dict(), r_rep)

    assert _abi.step_table(15.0 - 0.08).size == 49
    assert _long_score_ref(oracle, lr, 15.0)["ticks"][0][1].max() > 20   # cells in range at 15 m
    with _abi.Context(0) as ctx:
        ctx.set_terrain(lr.cloud, point_step=16)
        ctx.set_cells(lr.xyz, lr.nrm)
        for what, md in (("fan", 15.0), ("score", 15.0), ("score", 110.0), ("fan", 110.0),
                         ("fan", 15.0), ("score", 15.0), ("score", 77.6), ("fan", 77.6),
                         ("fan", 110.0), ("score", 110.0)):
            (fan_q if what == "fan" else score_q)(ctx, md)


@pytest.mark.parametrize("md", [15.0, 110.0])
@pytest.mark.parametrize("g", ["2", "4", "8", "16"])
def test_score_wide_lane_counts(oracle, long_range, g, md, monkeypatch):
    """PCP_SCORE_WIDE_G = 2 / 4 / 8 / 16 selects k_score_cells_wide<true, G> while the step
    table fits LDS (max_distance 15); past it (max_distance 110) only the 16-lane kernel exists
    and the launcher sizes its grid from the width it launches.  600 cells, so a grid sized for
    G < 16 lanes but run by the 16-lane kernel would score C G / 16 cells only.  The launcher
    did that before: at max_distance 110 this test failed on it for G = 2 / 4 / 8, with 1,020 /
    859 / 589 of the 3,000 pose cells and 303 / 255 / 177 of the 600 zx120 cells positive on
    one side only, in every row.  Every cell and row of pcp_score_matrix, and the totals, flags
    and covered counts of pcp_score_poses, against the oracle; totals under the exact bar
    (first MI355X run: 0 differ for every G; cells: 1 of 448 at 15 m, 7 of 1,996 at 110 m)."""
    lr = long_range
    ref = _long_score_ref(oracle, lr, md)
    monkeypatch.setenv("PCP_SCORE_WIDE_G", g)
    assert lr.xyz.shape[0] * 2 // 16 < lr.xyz.shape[0]
    with _abi.Context(0) as ctx:
        ctx.set_terrain(lr.cloud, point_step=16)
        ctx.set_cells(lr.xyz, lr.nrm)
        params = _abi.default_vl_params(max_distance=md)
        sm, sz = ctx.score_matrix(lr.score_poses, lr.zx, params)
        bad_m, bad_z = (sm > 0) != (ref["sm"] > 0), (sz > 0) != (ref["sz"] > 0)
        rows = np.flatnonzero(bad_m.any(1))
        assert rows.size == 0 and not bad_z.any(), (rows, int(bad_m.sum()), int(bad_z.sum()))
        _long_score_check(ctx, lr, ref, md, lr.score_poses, tag=f"G={g}")


@pytest.mark.parametrize("g", ["3", "32", "-1", "x", "0", "4x", ""])
def test_score_wide_lane_count_rejected(g, monkeypatch, capfd):
    """A PCP_SCORE_WIDE_G that is not one of the instantiated widths never reaches a launch:
    pcp_create returns PCP_E_INVALID and names the variable on stderr (no context exists to
    carry the message); with the variable unset again a context is created as usual."""
    monkeypatch.setenv("PCP_SCORE_WIDE_G", g)
    with pytest.raises(_abi.PcpError) as e:
        _abi.Context(0)
    assert e.value.code == _abi.PCP_E_INVALID
    assert "PCP_SCORE_WIDE_G" in capfd.readouterr().err
    monkeypatch.delenv("PCP_SCORE_WIDE_G")
    with _abi.Context(0) as ctx:
        assert ctx.cells_count() == 0


def test_step_table_upper_limit(oracle):
    """PCP_MAX_STEPS (include/pcp_abi.h): a max_distance whose step table is longer is refused
    with PCP_E_INVALID by the fan and by every scoring entry point before anything is launched
    (no terrain is set here, so nothing could march anyway) -- K = 32768, which an int16 first
    hit cannot hold, and K = PCP_MAX_STEPS + 1 -- and the context answers normal queries
    afterwards, the longest accepted table included."""
    M = _abi.MAX_STEPS
    md_of = lambda K: 0.5 + 0.3 * (K - 1) + 0.08 + 0.15   # s_{K-1} < md - 0.08 <= s_K
    for K in (32768, M + 1, M):
        assert _abi.step_table(md_of(K) - 0.08).size == K
    assert M <= 32767
    poses = np.array([[0.0, 0.0, 1.0, 0.0, 0.0], [3.0, 1.0, 2.0, 0.0, 1.0]])
    xyz = np.array([[2.0, 0.0, 0.5], [4.0, 1.0, 0.2], [900.0, 0.0, 1.0]])
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (3, 1))
    zx = np.array([0.0, 0.0, 2.0, 0.0, 0.0])
    bb = np.array([0.0, 4.0, -2.0, 2.0, 0.0, 1.0])

    def refused(call):
        with pytest.raises(_abi.PcpError) as e:
            call()
        assert e.value.code == _abi.PCP_E_INVALID and "PCP_MAX_STEPS" in str(e.value), e.value

    with _abi.Context(0) as ctx:
        ctx.set_cells(xyz, nrm)
        fan15 = _abi.fan_params(n_az=64, n_el=2)
        b0, u0, fh0, _ = ctx.raycast_fan(poses, fan15, want_first_hit=True)
        for K in (32768, M + 1):
            fan = _abi.fan_params(n_az=64, n_el=2, max_distance=md_of(K))
            vp = _abi.default_vl_params(max_distance=md_of(K), num_candidates=9)
            refused(lambda: ctx.raycast_fan(poses, fan, want_first_hit=True))
            refused(lambda: ctx.raycast_fan(poses, fan))
            refused(lambda: ctx.raycast_fan_stats(poses, fan))
            refused(lambda: ctx.raycast_fan_burst(poses, fan, reps=1))
            refused(lambda: ctx.score_poses(poses, zx, vp, np.zeros(3, np.uint8)))
            refused(lambda: ctx.score_matrix(poses, zx, vp))
            refused(lambda: ctx.score_poses_stats(poses, zx, vp))
            refused(lambda: ctx.score_poses_burst(poses, zx, vp, reps=1))
            refused(lambda: ctx.generate_and_score(bb, vp, zx, np.zeros(3, np.uint8)))
            # the cached (15 m) table is still the one in use
            b1, u1, fh1, _ = ctx.raycast_fan(poses, fan15, want_first_hit=True)
            np.testing.assert_array_equal(fh1, fh0)
            np.testing.assert_array_equal(u1, u0)
        assert (fh0 == -1).all() and u0.tolist() == [64 * 2 * 49] * 2
        # a normal scoring query, then the longest table that is accepted (md_of(M): ~1,229 m,
        # the cell at 900 m in range)
        fanM = _abi.fan_params(n_az=64, n_el=2, max_distance=md_of(M))
        bM, uM, fhM, _ = ctx.raycast_fan(poses, fanM, want_first_hit=True)
        assert bM.tolist() == [0, 0] and uM.tolist() == [64 * 2 * M] * 2 and (fhM == -1).all()
        for md, n_cov in ((15.0, 2), (md_of(M), 3)):
            fg = np.zeros(3, np.uint8)
            fr = fg.copy()
            tot, cov, rep = ctx.score_poses(poses, zx, _abi.default_vl_params(max_distance=md), fg)
            r_tot, r_cov, r_rep = oracle.score_poses(None, None, xyz, nrm, poses, zx,
                                                     oracle.vl_params(max_distance=md), fr)
            np.testing.assert_array_equal(fg, fr)
            np.testing.assert_array_equal(cov, r_cov)
            parity.assert_totals(tot, r_tot)
            assert r_cov.tolist() == [n_cov] * 2 and rep.total_cells == 3


def _need_devices(devices):
    if len(set(devices)) > 1 and _abi.device_count() < len(set(devices)):
        pytest.skip(f"needs {len(set(devices))} GPUs (RCCL over distinct devices); "
                    f"{_abi.device_count()} visible")


def test_multi_rejects_mixed_device_lists(gpu):
    """Devices all distinct (RCCL) or all the same (on-device combine); a mixed list such as
    {0, 0, 1} would combine buffers across devices without peer access: refused."""
    with pytest.raises(_abi.PcpError):
        _abi.Multi([0, 0, 1])
    with pytest.raises(_abi.PcpError):
        _abi.Multi([0, 1, 1])


@pytest.mark.parametrize("devices", [[0], [0, 0, 0], [0, 1], [0, 1, 2, 3]])
def test_multi_fan_matches_single_context(gpu, loaded, scene, devices):
    """pcp_multi: the C2 poses sharded over the ranks, ONE all-reduce(MIN) over
    the (blocked << 32) | pose keys -- RCCL over one device, or three ranks sharing device 0
    (keys combined on the device) -- bit-identical to one context over all poses."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import bench

    _need_devices(devices)
    poses, _ = bench._poses_for(gpu, bench._grid_bbox(scene.area), scene.zx120_pose5, 256)
    fan = _abi.fan_params()
    b1, u1, _, best1 = gpu.raycast_fan(poses, fan)
    with _abi.Multi(devices) as m:
        assert m.n == len(devices) and m.uses_rccl == (len(set(devices)) == len(devices))
        m.set_terrain(scene.terrain, point_step=32)
        for sel in (poses, poses[:5], poses[:1]):        # ranks with 0 poses too
            b, u, best = m.raycast_fan(sel, fan)
            n = sel.shape[0]
            np.testing.assert_array_equal(b, b1[:n])
            np.testing.assert_array_equal(u, u1[:n])
            assert best == int(np.argmin(b1[:n]))
        b, u, best = m.raycast_fan(poses[:0], fan)
        assert b.size == 0 and best == -1
    assert best1 == int(np.argmin(b1))


@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 1]])
def test_multi_score_matches_single_context(gpu, loaded, scene, cells, aux, devices):
    """pcp_multi_score_poses: totals, covered counts, strict-'>' best index, stale flags and the
    colour report over two ticks (the second starting from the first's flags), identical to
    pcp_score_poses on one context."""
    _need_devices(devices)
    params = _abi.default_vl_params()
    poses = gpu.generate_candidates(cells.grid_bbox, _abi.default_vl_params(num_candidates=400),
                                    scene.zx120_pose5)
    with _abi.Multi(devices) as m:
        m.set_terrain(scene.terrain, point_step=32)
        m.set_aux_cloud(aux, point_step=32)
        m.set_cells(cells.xyz, cells.normals)
        f1 = np.zeros(cells.xyz.shape[0], np.uint8)
        fm = f1.copy()
        for sel in (poses, poses[::7][:3], poses[:0]):
            t1, c1, r1 = gpu.score_poses(sel, scene.zx120_pose5, params, f1)
            tm, cm, rm = m.score_poses(sel, scene.zx120_pose5, params, fm)
            np.testing.assert_array_equal(tm, t1)
            np.testing.assert_array_equal(cm, c1)
            np.testing.assert_array_equal(fm, f1)
            assert rm.as_dict() == r1.as_dict()


def test_gpu_matches_flann_restatement(gpu, oracle, loaded, scene):
    """The GPU's first hits against the oracle in FLANN mode (oracle/pcp_flann.c: the
    KdTreeFLANN search the reference runs, float pruning included) on 8 of the C2 poses,
    every sample query also cross-checked against the exact grid count."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import bench

    poses, _ = bench._poses_for(gpu, bench._grid_bbox(scene.area), scene.zx120_pose5, 256)
    sel = poses[::32]
    fan = _abi.fan_params()
    blocked, units, fh, _ = gpu.raycast_fan(sel, fan, want_first_hit=True)
    T, _ = loaded
    tree = oracle.KdTree(scene.terrain)
    oracle.set_threads(16)
    try:
        rb, ru, rfh, st = oracle.raycast_fan_kd(tree, T, sel, 1024, 256, fan.el_min, fan.el_max,
                                                fan.max_distance)
    finally:
        oracle.set_threads(1)
    assert st["count_mismatch"] == 0 and st["any_mismatch"] == 0, st
    assert st["queries"] == int(ru.sum())
    np.testing.assert_array_equal(fh, rfh)
    np.testing.assert_array_equal(blocked, rb)
    np.testing.assert_array_equal(units, ru)
