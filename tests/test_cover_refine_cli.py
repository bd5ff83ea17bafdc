"""`pcp_nodes_cli cover_refine` on the GPU -- CoveragePlacement::refine over the real library: the
files it writes and the JSON line it prints against the NumPy restatement
(tests/cover_refine_ref.py), greedy's answer refined in the same process when no start is given,
the log's line per move, and the status-2 refusals of bad arguments."""
import json
import subprocess
from pathlib import Path

import cover_ref
import cover_refine_ref
import numpy as np
import pytest

from pointcloud_processor_amd import _abi

CLI = _abi.LIB_PATH.parent / "pcp_nodes_cli"


def _records32(cloud):
    """The terrain as the CLI reads it: 32-byte records, x / y / z at 0 / 4 / 8, a tag behind."""
    rec = np.zeros((cloud.shape[0], 8), np.float32)
    rec[:, :3] = cloud[:, :3]
    rec[:, 5] = np.arange(cloud.shape[0], dtype=np.float32)
    return rec


def _run(args, timeout=120):
    return subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, text=True,
                          timeout=timeout)


# (roi, separation, KMAX, --start, --locked, --max-moves, FIXED)
CASES = [("box_a", 0.0, 2, None, None, None, ()),          # greedy's pair becomes the exact pair
         ("all", cover_ref.SEP, 4, [0, 1, 2, 3], None, None, ()),   # six moves, two slots twice
         ("xpos", 0.0, 3, [3, 2, 1, 0], 2, 1, ()),         # locked slots, the moves run out
         ("all", cover_ref.SEP, 2, None, None, None, (10, 40))]     # FIXED in front, locked


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_cli_cover_refine_is_the_restatement(oracle, tmp_path: Path, case):
    roi_name, sep, kmax, start, locked, max_moves, fixed = case
    inst = cover_ref.instance(oracle)
    roi = cover_refine_ref.rois(oracle)[roi_name]
    if start is None:   # greedy's answer beside FIXED, those in front and locked
        g = cover_ref.greedy(inst["seen"], inst["poses"][:, :2], inst["N"], kmax, sep, fixed, roi)
        want_start = list(fixed) + g["selected"].tolist()
        want_locked = len(fixed)
    else:
        want_start, want_locked = start, locked or 0
    ref = cover_refine_ref.refine(inst["seen"], inst["poses"][:, :2], inst["N"], want_start,
                                  want_locked, 16 if max_moves is None else max_moves, sep, roi)
    rec = _records32(inst["cloud"])
    (tmp_path / "terrain.f32").write_bytes(rec.tobytes())
    (tmp_path / "poses.f64").write_bytes(np.ascontiguousarray(inst["poses"]).tobytes())
    roi_arg = "-"
    if roi is not None:
        (tmp_path / "roi.u8").write_bytes(roi.tobytes())
        roi_arg = tmp_path / "roi.u8"
    args = ["cover_refine", tmp_path / "terrain.f32", inst["N"], tmp_path / "poses.f64", 100, 37,
            15.0, kmax, sep, roi_arg, tmp_path / "sel.i64", tmp_path / "owner.i32",
            tmp_path / "blind.f32"]
    if fixed:
        args.append(",".join(str(f) for f in fixed))
    if start is not None:
        args += ["--start", ",".join(str(p) for p in start)]
    if locked is not None:
        args += ["--locked", locked]
    if max_moves is not None:
        args += ["--max-moves", max_moves]
    r = _run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    sel = np.fromfile(tmp_path / "sel.i64", np.int64).reshape(-1, 3)
    owner = np.fromfile(tmp_path / "owner.i32", np.int32)
    blind = np.fromfile(tmp_path / "blind.f32", np.float32).reshape(-1, 8)
    # the rounds: the slots in order, each with the points it owns
    own = [int(np.count_nonzero(ref["point_owner"] == i)) for i in range(len(want_start))]
    assert sel[:, 0].tolist() == ref["selected"].tolist() and sel[:, 1].tolist() == own
    assert sel[:, 2].tolist() == np.cumsum(own).tolist() and sel[-1, 2] == ref["covered"]
    np.testing.assert_array_equal(owner, ref["point_owner"])
    in_roi = np.ones(inst["N"], bool) if roi is None else roi != 0
    want_blind = rec[in_roi & (ref["point_owner"] == cover_refine_ref.OWNER_NONE)]
    assert blind.tobytes() == want_blind.tobytes()
    moves = [list(m) for m in zip(ref["move_slot"].tolist(), ref["move_from"].tolist(),
                                  ref["move_to"].tolist(), ref["move_covered"].tolist())]
    assert out == {"n_candidates": 71, "n_selected": len(want_start), "n_points": inst["N"],
                   "roi_points": ref["roi_points"], "base_covered": 0, "covered": ref["covered"],
                   "n_blind": want_blind.shape[0], "n_locked": want_locked,
                   "start_covered": ref["start_covered"], "moves": moves,
                   "converged": ref["converged"]}
    assert ref["roi_points"] - ref["covered"] == want_blind.shape[0]
    # the table goes to stderr, with a line per move
    assert f"Coverage Placement (0 Fixed + {len(want_start)} Mobile)" in r.stderr
    assert f"Exchange refinement ({want_locked} locked): start {ref['start_covered']} points" in r.stderr
    for i, (slot, frm, to, cov) in enumerate(moves):
        assert f"  Move {i + 1}: slot {slot}, candidate {frm} -> {to}, covered {cov} (" in r.stderr
    tail = "No single move adds a point" if ref["converged"] else "Moves ran out"
    assert f"  {tail} after {len(moves)} move" in r.stderr
    if roi_name == "box_a":
        assert ref["selected"].tolist() == [43, 50] and ref["covered"] == 2330
    if max_moves == 1:
        assert ref["converged"] == 0 and len(moves) == 1


@pytest.mark.gpu
def test_cli_cover_refine_refuses_bad_arguments(tmp_path: Path):
    cloud = np.zeros((4, 8), np.float32)
    cloud[:, 0] = np.arange(4)
    (tmp_path / "t.f32").write_bytes(cloud.tobytes())
    (tmp_path / "roi3.u8").write_bytes(bytes([1, 1, 1]))
    outs = [tmp_path / "s", tmp_path / "o", tmp_path / "b"]
    base = ["cover_refine", tmp_path / "t.f32", 4, "0,0,1,0,0,1,1,1,0,0", 8, 2, 5.0, 1, 0.0]
    assert _run(base[:9] + ["-"] + outs[:2]).returncode == 2                 # too few arguments
    bad_poses = list(base)
    bad_poses[3] = "0,0,1,0"
    assert _run(bad_poses + ["-"] + outs).returncode == 2                    # not 5 per candidate
    assert _run(base + [tmp_path / "roi3.u8"] + outs).returncode == 2        # ROI bytes != TN
    assert _run(base + ["-"] + outs + ["2"]).returncode == 2                 # FIXED is no candidate
    assert _run(base + ["-"] + outs + ["--start", "0,2"]).returncode == 2    # START is no candidate
    assert _run(base + ["-"] + outs + ["--start", "0.5"]).returncode == 2
    assert _run(base + ["-"] + outs + ["--start"]).returncode == 2           # no value
    assert _run(base + ["-"] + outs + ["0", "--start", "1"]).returncode == 2   # FIXED with START
    assert _run(base + ["-"] + outs + ["--locked", "x"]).returncode == 2
    assert _run(base + ["-"] + outs + ["--max-moves", "65"]).returncode == 2
    assert _run(base + ["-"] + outs + ["--moves", "3"]).returncode == 2      # no such option
    assert _run(base + ["-"] + outs + ["--start", "0", "1"]).returncode == 2   # a stray argument
    for p in outs:
        assert not p.exists()
    assert _run(["cover_refine"]).returncode == 2
