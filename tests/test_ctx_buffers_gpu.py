"""The context's owning buffers on the GPU: pcp_filter_merge of 1, then 3, then 1 cloud in ONE
context grows ctx->fbuf by a vector resize while the first cloud's scratch holds device memory, so
CloudBufs that own memory are moved; then contexts are created and destroyed used and unused
(~pcp_ctx with and without a single allocation).  Every call's bytes equal those of a fresh
context given the same call, and the oracle's (crop + VoxelGrid + transform)."""
import numpy as np
import pytest

from pointcloud_processor_amd import _abi, synth

pytestmark = pytest.mark.gpu

BOX = np.array([0.0, 15.0, -10.0, 10.0, -1.5, 10.0])
LEAF = 0.05
IDENTITY = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _tf(i):
    s, c = np.sin(0.15 * i), np.cos(0.15 * i)
    return (0.5 * i, -0.25 * i, 0.1 * i), (0.0, 0.0, s, c) if i % 2 else (0.0, s, 0.0, c)


def _ref(oracle, clouds, tfs, rgbs):
    parts = []
    for cloud, tf, rgb in zip(clouds, tfs, rgbs):
        kept = oracle.crop_box(cloud, BOX)
        v, _, _, pt = oracle.voxel_grid(cloud[kept], LEAF)
        assert not pt
        parts.append(oracle.transform_rgb(v, *tf, rgb))
    return np.concatenate(parts), [p.shape[0] for p in parts]


def test_fbuf_grows_with_live_scratch_then_contexts_close(oracle):
    clouds = [synth.lidar_cloud(300 + 7 * i, seed=310 + i, sensor_height=2.0 + 0.5 * i)
              for i in range(3)]
    tfs = [IDENTITY, _tf(1), _tf(2)]          # identity and two non-identity transforms
    rgbs = [(10, 200, 30), (250, 0, 7), (1, 2, 3)]
    calls = [(0,), (0, 1, 2), (2,)]           # 1 cloud, 3 clouds (the resize), 1 cloud again
    args = [([clouds[i] for i in c], [BOX] * len(c), LEAF, [tfs[i] for i in c],
             [rgbs[i] for i in c]) for c in calls]
    refs = [_ref(oracle, a[0], a[3], a[4]) for a in args]
    assert all(min(per) > 0 for _, per in refs)

    ctx = _abi.Context(0)
    got = [ctx.filter_merge(*a) for a in args]
    ctx.close()
    for a, (out, per), (ref, per_ref) in zip(args, got, refs):
        assert list(per) == per_ref
        np.testing.assert_array_equal(_u32(out[:, :5]), _u32(ref[:, :5]))
        with _abi.Context(0) as fresh:        # a fresh context given the same call
            out1, per1 = fresh.filter_merge(*a)
        assert list(per1) == list(per)
        np.testing.assert_array_equal(_u32(out1), _u32(out))

    _abi.Context(0).close()                   # created and closed without any call
    with _abi.Context(0) as last:             # created, used once, closed
        out, per = last.filter_merge(*args[1])
    np.testing.assert_array_equal(_u32(out), _u32(got[1][0]))
