"""The library's SE(3) under roll and pitch (rigid_ref.py's quaternions: all four components
non-zero, w < 0, next to pi, not of unit length, zero, gimbal lock), where every transform the
suite fed it before was a rotation about one axis: pcp_transform_concat on both staging paths
(the pinned one-launch k_xform_batch and the DMA'd k_xform_raw), its record layouts, block
tiles, empty clouds and capacity; the filter chains' three emit kernels; the drivable grid;
the carve's pose (tf2's setRotation / getRPY) and its generated-lattice cache.

Everything is bit-exact against the CPU oracle as uint32 words; a transform by a unit q is
also within rigid_ref.bound() of the float64 cross-product reference, which shares no formula
with the oracle.  test_rigid_ref.py shows on the CPU that these inputs catch a wrong sign, a
transposed entry, a fused product and a re-associated sum, and that a yaw catches none."""
import ctypes as C

import numpy as np
import pytest

import carve_cases as cc
import rigid_ref as rr
from pointcloud_processor_amd import _abi, synth
from test_carve_edges import _compare

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0xA5A5A5A5)
NAMES = list(rr.QUATS)
BOX = np.array([0.0, 15.0, -10.0, 10.0, -1.5, 10.0])
LEAF = 0.05


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ctx(monkeypatch, var, value):
    if value is None:
        monkeypatch.delenv(var, raising=False)
    else:
        monkeypatch.setenv(var, str(value))
    return _abi.Context(0)


@pytest.fixture(scope="module")
def paths():
    """{"pinned": the default context (PCP_ZC_IN unset: inputs up to 4 MiB and 8 clouds are
    read in place by k_xform_batch), "dma": a context created under PCP_ZC_IN=0 (every call
    through k_xform_raw)}."""
    with pytest.MonkeyPatch.context() as mp:
        ctxs = {"pinned": _ctx(mp, "PCP_ZC_IN", None), "dma": _ctx(mp, "PCP_ZC_IN", 0)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.fixture(scope="module")
def cloud():
    c = rr.cloud()
    c.flags.writeable = False
    return c


def _concat(ctx, views, tfs, rgbs, cap=None):
    """One raw pcp_transform_concat call into a sentinel-filled buffer of cap + 1 records ->
    (rc, n_out, the buffer as (cap + 1, 8) uint32)."""
    k = len(views)
    varr = (_abi.CloudView * max(k, 1))(*views)
    total = sum(v.n for v in views)
    cap = total if cap is None else cap
    out = np.full((cap + 1, 8), SENTINEL, np.uint32)
    rgb = np.ascontiguousarray(np.asarray(rgbs, np.uint8).reshape(-1))
    n = C.c_uint64(0xDEAD)
    rc = ctx.lib.pcp_transform_concat(ctx.h, k, varr, ctx._rigids(tfs), rgb.ctypes.data,
                                      out.ctypes.data, cap, C.byref(n))
    return rc, n.value, out


def _reference(oracle, clouds, tfs, rgbs):
    parts = [oracle.transform_rgb(c, t, q, rgb) for c, (t, q), rgb in zip(clouds, tfs, rgbs)
             if c.shape[0]]
    return np.concatenate(parts) if parts else np.zeros((0, 8), np.float32)


def _within_bound(got, clouds, tfs, names):
    """The records of every cloud under a unit q against the float64 reference."""
    at = 0
    for c, (t, q), name in zip(clouds, tfs, names):
        n = c.shape[0]
        if n and name in rr.UNIT:
            worst = rr.units(got[at:at + n].view(np.float32), c, t, q)
            print(f"{name}: {worst:.2f} of the bound over {n} points")
            assert worst <= 1.0
        at += n


# ---------------------------------------------------------------- 1: every quaternion
@pytest.mark.parametrize("name", NAMES)
def test_transform_concat_every_quaternion(gpu, oracle, cloud, name):
    """10,007 points of [-50, 50]^3, a translation no float holds: x, y, z and the constant
    words bit-exact, the colour word b | g << 8 | r << 16 | 255 << 24 for three colours."""
    t, q = rr.T_TILT, rr.QUATS[name]
    for rgb in ((0, 0, 0), (255, 255, 255), (1, 2, 3)):
        rc, n, out = _concat(gpu, [_abi.cloud_view(cloud)], [(t, q)], [rgb])
        assert rc == _abi.PCP_OK and n == rr.N_CLOUD
        np.testing.assert_array_equal(out[:n], _u32(oracle.transform_rgb(cloud, t, q, rgb)))
        assert np.all(out[:n, 4] == rr.colour_word(rgb)) and np.all(out[n] == SENTINEL)
    _within_bound(out[:n], [cloud], [(t, q)], [name])


# ---------------------------------------------------------------- 2: both staging paths
COUNTS = {
    "k9": [300, 1, 257, 700, 64, 1000, 511, 2, 129],   # k > kXfMax = 8: the DMA path by k
    "over_4mib": [262_145],     # the smallest count of 16-byte records staged past 4 MiB
    "block_edges": [1, 255, 256, 257, 513],            # tile0[] around the 256-thread block
    "empty_first": [0, 300, 257],
    "empty_middle": [300, 0, 257],
    "empty_last": [300, 257, 0],
    "k1": [1000],
    "k0": [],
    "all_empty": [0, 0, 0],
}


def _inputs(counts):
    """Cloud i: counts[i] points, its own quaternion of the list, translation and colour."""
    k = len(counts)
    names = [NAMES[i % len(NAMES)] for i in range(k)]
    clouds = [rr.cloud(n, seed=10 + i) for i, n in enumerate(counts)]
    tfs = [(rr.translation(i), rr.QUATS[nm]) for i, nm in enumerate(names)]
    rgbs = [((37 * i + 1) % 256, (91 * i + 5) % 256, (13 * i + 200) % 256) for i in range(k)]
    return clouds, tfs, rgbs, names


@pytest.mark.parametrize("case", list(COUNTS))
def test_transform_concat_both_paths(paths, oracle, case):
    """The same inputs through the default context and one created under PCP_ZC_IN=0: the
    oracle's bytes from both, nothing written past the last record."""
    clouds, tfs, rgbs, names = _inputs(COUNTS[case])
    ref = _u32(_reference(oracle, clouds, tfs, rgbs))
    total = sum(COUNTS[case])
    assert ref.shape[0] == total
    views = [_abi.cloud_view(c) for c in clouds]
    for path, ctx in paths.items():
        rc, n, out = _concat(ctx, views, tfs, rgbs)
        assert rc == _abi.PCP_OK and n == total, path
        np.testing.assert_array_equal(out[:n], ref, err_msg=path)
        assert np.all(out[n:] == SENTINEL), path
    _within_bound(out[:total], clouds, tfs, names)


@pytest.mark.parametrize("zc,case,dma", [(None, "k1", False), (None, "block_edges", False),
                                         (None, "k9", True), (None, "over_4mib", True),
                                         (0, "k1", True)])
def test_what_selects_the_path(zc, case, dma, monkeypatch):
    """The two paths seen from outside, in the process's device allocations (pcp_alloc_stats)
    over the first call of a fresh context: the pinned path stages, runs and lands in pinned
    memory and allocates no device buffer; the DMA path allocates its staging and its output
    buffer -- under PCP_ZC_IN=0, with more than 8 clouds, and past 4 MiB of input."""
    clouds, tfs, rgbs, _ = _inputs(COUNTS[case])
    with _ctx(monkeypatch, "PCP_ZC_IN", zc) as ctx:
        before = _abi.alloc_stats()["device"]
        rc, n, _ = _concat(ctx, [_abi.cloud_view(c) for c in clouds], tfs, rgbs)
        grew = _abi.alloc_stats()["device"] - before
    assert rc == _abi.PCP_OK and n == sum(COUNTS[case])
    assert (grew > 0) == dma, grew


# ---------------------------------------------------------------- 3: record layouts
LAYOUTS = [(12, (0, 4, 8)), (32, (16, 20, 24)), (20, (4, 8, 0)), (16, (0, 4, 8))]


def _pack(c, step, offs):
    """The points as raw records: x, y, z at offs, every other byte 0xA5."""
    raw = np.full((c.shape[0], step), 0xA5, np.uint8)
    for a in range(3):
        raw[:, offs[a]:offs[a] + 4] = c[:, a:a + 1].copy().view(np.uint8)
    return raw


def test_transform_concat_layouts(paths, oracle):
    """point_step 12 packed, 32 with x, y, z at 16, 20, 24, 20 with the fields in the order z,
    x, y (and the float4 fast path's 16) mixed in one call, on both paths."""
    clouds, tfs, rgbs, _ = _inputs([1000, 257, 513, 300])
    raws = [_pack(c, step, offs) for c, (step, offs) in zip(clouds, LAYOUTS)]
    views = [_abi.cloud_view(r, step, offs) for r, (step, offs) in zip(raws, LAYOUTS)]
    ref = _u32(_reference(oracle, clouds, tfs, rgbs))
    for path, ctx in paths.items():
        rc, n, out = _concat(ctx, views, tfs, rgbs)
        assert rc == _abi.PCP_OK and n == ref.shape[0], path
        np.testing.assert_array_equal(out[:n], ref, err_msg=path)


@pytest.mark.parametrize("step,offs", [(16, (0, 4, 10)), (16, (2, 4, 8)), (8, (0, 4, 4))])
def test_transform_concat_refuses_bad_layouts(paths, step, offs):
    """A misaligned offset and point_step = 8: PCP_E_INVALID, the output untouched -- also
    where the bad view follows a good one."""
    clouds, tfs, rgbs, _ = _inputs([300, 257])
    good = _abi.cloud_view(clouds[0])
    bad = _abi.cloud_view(_pack(clouds[1], 16, (0, 4, 8)), step, offs)
    for path, ctx in paths.items():
        for views in ([good, bad], [bad, good]):
            rc, _, out = _concat(ctx, views, tfs, rgbs)
            assert rc == _abi.PCP_E_INVALID and np.all(out == SENTINEL), path


# ---------------------------------------------------------------- 4: capacity
def test_transform_concat_capacity(paths, oracle):
    """cap = total - 1: PCP_E_CAPACITY, *n_out = total, not a byte written; cap = total on the
    next call succeeds."""
    clouds, tfs, rgbs, _ = _inputs([300, 257, 513])
    views = [_abi.cloud_view(c) for c in clouds]
    ref = _u32(_reference(oracle, clouds, tfs, rgbs))
    total = ref.shape[0]
    for path, ctx in paths.items():
        rc, n, out = _concat(ctx, views, tfs, rgbs, cap=total - 1)
        assert rc == _abi.PCP_E_CAPACITY and n == total and np.all(out == SENTINEL), path
        rc, n, out = _concat(ctx, views, tfs, rgbs, cap=total)
        assert rc == _abi.PCP_OK and n == total, path
        np.testing.assert_array_equal(out[:n], ref, err_msg=path)


# ---------------------------------------------------------------- 5: non-finite input
def test_transform_concat_non_finite(paths, oracle):
    """NaN, +inf and -inf in one coordinate of a row, under `tilt` (no zero entry: the bad value
    reaches every output), and rows with x and y both infinite (inf - inf: a NaN the transform
    makes itself).  The output's NaN mask is the oracle's and every other word its bits.  NaN
    payloads and signs are not compared: x86 and the device quiet and propagate them
    differently, and the reference's consumers only ask isfinite."""
    c = rr.cloud(11 * 40 + 57, seed=30).copy()
    for kind, bad in enumerate((np.nan, np.inf, -np.inf)):
        for a in range(3):
            lo = (3 * kind + a) * 40
            c[lo:lo + 40, a] = bad
    c[360:440, 0] = np.inf
    c[360:400, 1], c[400:440, 1] = np.inf, -np.inf
    t, q, rgb = rr.T_TILT, rr.QUATS["tilt"], (9, 8, 7)
    ref = oracle.transform_rgb(c, t, q, rgb)
    nan = np.isnan(ref)
    assert nan[:120, :3].all() and np.isinf(ref[120:360, :3]).all() and not nan[120:360].any()
    assert nan[360:440, :3].any() and np.isinf(ref[360:440, :3]).any() and not nan[440:].any()
    for path, ctx in paths.items():
        rc, n, out = _concat(ctx, [_abi.cloud_view(c)], [(t, q)], [rgb])
        assert rc == _abi.PCP_OK and n == c.shape[0], path
        got = out[:n]
        np.testing.assert_array_equal(np.isnan(got.view(np.float32)), nan, err_msg=path)
        np.testing.assert_array_equal(got[~nan], _u32(ref)[~nan], err_msg=path)


# ---------------------------------------------------------------- 6: the filter chains' emits
def _chain_tfs(k):
    names = [("tilt", "non_unit_big")[i % 2] for i in range(k)]
    return [(rr.translation(i), rr.QUATS[nm]) for i, nm in enumerate(names)]


def _rgbs(k):
    return [((37 * i) % 256, (91 * i + 5) % 256, (13 * i + 200) % 256) for i in range(k)]


def _ref_voxels(oracle, c, leaf):
    kept = oracle.crop_box(c, BOX)
    v, _, _, passthrough = oracle.voxel_grid(c[kept], leaf)
    assert kept.size and not passthrough
    return v, kept.size


def _ref_merged(oracle, clouds, leaf, tfs, rgbs):
    vox = [_ref_voxels(oracle, c, leaf) for c in clouds]
    parts = [oracle.transform_rgb(v, t, q, rgb) for (v, _), (t, q), rgb in zip(vox, tfs, rgbs)]
    return np.concatenate(parts), vox


@pytest.fixture(scope="module")
def scans():
    return [synth.lidar_cloud(30_000, seed=171),
            synth.lidar_cloud(30_000, seed=172, sensor_height=3.5)]


@pytest.fixture(scope="module")
def scans_ref(scans, oracle):
    return _ref_merged(oracle, scans, LEAF, _chain_tfs(2), _rgbs(2))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_filter_merge_every_chain(scans, scans_ref, mode, monkeypatch):
    """pcp_crop_voxel, then pcp_filter_merge under `tilt` and `non_unit_big`: the general (0)
    and the LSD fast chain (1) emit from k_seg_centroid, the bucket chain (2) from k_bk_emit
    (no redo: it ran to its end)."""
    ref, vox = scans_ref
    tfs, rgbs = _chain_tfs(2), _rgbs(2)
    with _ctx(monkeypatch, "PCP_FM_FAST", mode) as ctx:
        out, ncrop = ctx.crop_voxel(scans[0], BOX, LEAF)
        assert ncrop == vox[0][1]
        np.testing.assert_array_equal(_u32(out[:, :3]), _u32(vox[0][0]))
        merged, per = ctx.filter_merge(scans, [BOX, BOX], LEAF, tfs, rgbs)
        assert ctx.profile_get("voxel_redo")[1] == 0
    assert list(per) == [v.shape[0] for v, _ in vox]
    np.testing.assert_array_equal(_u32(merged), _u32(ref))


@pytest.mark.parametrize("mode", [None, 0])
def test_filter_merge_nodes_tilted(scans, scans_ref, oracle, mode, monkeypatch):
    """pcp_filter_merge_nodes: the bucket chain's k_bk_emit by default, the general chain with
    a separate k_emit_rgb under PCP_FM_FAST=0."""
    ref, vox = scans_ref
    with _ctx(monkeypatch, "PCP_FM_FAST", mode) as ctx:
        merged, filt, crop = ctx.filter_merge_nodes(scans, [BOX, BOX], LEAF, _chain_tfs(2),
                                                    _rgbs(2))
        assert ctx.profile_get("voxel_redo")[1] == 0
    np.testing.assert_array_equal(_u32(merged), _u32(ref))
    for f, m, (v, ncrop) in zip(filt, crop, vox):
        assert int(m) == ncrop
        np.testing.assert_array_equal(_u32(f[:, :3]), _u32(v))


def test_filter_merge_two_batches_tilted(gpu, oracle):
    """Nine clouds: two launch batches, the general chain and a separate k_emit_rgb."""
    clouds = [synth.lidar_cloud(30_000, seed=180 + i, sensor_height=2.0 + 0.25 * i)
              for i in range(9)]
    tfs, rgbs = _chain_tfs(9), _rgbs(9)
    ref, vox = _ref_merged(oracle, clouds, LEAF, tfs, rgbs)
    out, per = gpu.filter_merge(clouds, [BOX] * 9, LEAF, tfs, rgbs)
    assert list(per) == [v.shape[0] for v, _ in vox]
    np.testing.assert_array_equal(_u32(out), _u32(ref))


# ---------------------------------------------------------------- 7: the drivable grid
@pytest.fixture(scope="module")
def drive():
    c = rr.drive_cloud()
    assert c.shape[0] == 20_000 and np.nanmin(c[:, 2]) < -1.4 and np.nanmax(c[:, 2]) > 1.4
    assert np.nanmax(np.abs(c[:, 2])) <= 1.55
    return c


@pytest.mark.parametrize("name", ["tilt", "neg_w", "non_unit_small"])
def test_drivable_area_tilted(gpu, oracle, drive, name):
    """Grid and origin bit-exact under roll and pitch.  On the oracle's own grids: every kind
    of cell occurs, and the grid differs from the one under the yaw of the same rotation alone
    -- the roll and pitch terms decide cells."""
    t, q = rr.T_TILT, rr.QUATS[name]
    grid, origin = gpu.drivable_area(drive, (t, q), rr.DRIVE_ROBOT, rr.DRIVE_START,
                                     _abi.drivable_params(**rr.DRIVE_KW))
    ref, r_origin = rr.drive_oracle(oracle, drive, t, q)
    np.testing.assert_array_equal(origin.view(np.uint64), r_origin.view(np.uint64))
    assert grid.shape == ref.shape == (60, 80) and grid.dtype == ref.dtype == np.int8
    np.testing.assert_array_equal(grid, ref)
    assert {-1, 0, 100} <= set(np.unique(ref).tolist())
    s = {"non_unit_small": 0.6}.get(name, 1.0)
    flat, _ = rr.drive_oracle(oracle, drive, t, rr.scaled(rr.TILT_YAW_ONLY, s))
    print(f"{name}: {(flat != ref).sum()} of {ref.size} cells differ from the yaw-only grid")
    assert (flat != ref).any()


# ---------------------------------------------------------------- 8: the carve's pose
def _excavate(ctx, q):
    return ctx.excavate(rr.carve_cloud(), (rr.CARVE_T, q), _abi.excavation_params(**rr.CARVE_KW))


def _check_carve(ctx, oracle, q):
    ref = rr.carve_reference(oracle, q)
    terr, area, pose = _excavate(ctx, q)
    _compare(terr, area, pose, rr.carve_cloud(), ref)
    g = cc.geometry(rr.CARVE_T, q, rr.CARVE_KW)
    assert (pose[0], pose[1], pose[3]) == (g.cx, g.cy, g.yaw)
    return ref, (terr, area, pose)


@pytest.mark.parametrize("name", ["tilt", "neg_w", "non_unit_big", "gimbal"])
def test_excavate_tilted_pose(gpu, oracle, name):
    """pose_out, kept points, generated surface and area records bit-exact with the oracle, the
    pose also with carve_cases.geometry(): -asin and / cos(pitch) of a pitched matrix, d != 1,
    w < 0, and the |m20| >= 1 branch."""
    q = rr.QUATS[name]
    ref, (_, _, pose) = _check_carve(gpu, oracle, q)
    keep = ref[0]
    if name == "gimbal":
        p = _abi.excavation_params(**rr.CARVE_KW)
        assert pose[3] == 0.0 and not np.signbit(pose[3])
        assert (pose[0], pose[1]) == (rr.CARVE_T[0], p.offset_y + rr.CARVE_T[1])
    elif name == "tilt":
        assert 0 < keep.sum() < keep.size
        assert abs(pose[3] - np.radians(20.0)) < 1e-12   # getRPY gives setRPY's yaw back
    elif name == "neg_w":
        tilt = rr.carve_reference(oracle, rr.QUATS["tilt"])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ref, tilt))


def test_excavate_lattice_cache_across_poses(oracle):
    """One context through tilt, -tilt, tilt (one pose three times: the generated lattice is
    reused), 2 tilt, the gimbal pose (another centre and yaw: regenerated) and tilt again
    (regenerated back): each call the oracle's bytes, the tilt calls all the same bytes."""
    tilt = rr.QUATS["tilt"]
    with _abi.Context(0) as ctx:
        first = None
        for q in (tilt, rr.QUATS["neg_w"], tilt, rr.scaled(tilt, 2.0), rr.QUATS["gimbal"], tilt):
            _, got = _check_carve(ctx, oracle, q)
            if q == rr.QUATS["gimbal"]:
                assert (got[2][0], got[2][1], got[2][3]) != (first[2][0], first[2][1], first[2][3])
                continue
            first = first or got
            for a, b in zip(got, first):
                assert a.tobytes() == b.tobytes()
