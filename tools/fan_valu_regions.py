"""VALU lines per region of the production fan kernel, from the device assembly of pcp_fan.hip
(hipcc with the Makefile's FLAGS plus --cuda-device-only -S; it cross-compiles without a GPU).

    python tools/fan_valu_regions.py fan.s [MANGLED_KERNEL_NAME]

Regions by the compiler's own loop comments: the pose loop is the kernel's depth-1 loop that holds
a depth-2 loop (the probe loop), whose depth-3 loops are the walks.  Inside the probe loop the
probe trip ends at the first branch (the candidate test); the rest of the depth-2 body that is no
walk is the candidate block.  Everything of the pose loop outside the probe loop is the per-pose
preamble and epilogue.  Counted: lines whose mnemonic starts with v_ (v_readlane / v_writelane /
v_readfirstlane among them; they issue on the VALU pipe), and those three and v_pk_* on their own."""
import re
import sys

DEFAULT = "_ZN3pcp17k_raycast_fan_xcdILi0ELi64ELb1ELi8ELi8ELb1ELi8ELb0ELb1EEEvNS_7FanArgsEj"


def kernel_lines(path, name):
    out, on = [], False
    for line in open(path):
        if line.startswith(name + ":"):
            on = True
        if on:
            out.append(line.rstrip("\n"))
            if "s_endpgm" in line:
                break
    if not out:
        raise SystemExit(f"{name}: not in {path}")
    return out


def regions(lines):
    """label each instruction line with its region"""
    # block -> depth from the "in Loop: Header=... Depth=n" / "Loop Header: Depth=n" comments
    depth, cur = {}, None
    block_of = []
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", l) or re.match(r"^; %bb\.(\d+):", l)
        if m:
            cur = m.group(1)
            d = re.search(r"Depth=(\d+)", l)
            depth[cur] = int(d.group(1)) if d else 0
        elif cur is not None and "Loop Header: Depth=" in l:
            depth[cur] = int(re.search(r"Depth=(\d+)", l).group(1))
        block_of.append(cur)
    # the pose loop: first depth-1 block whose header comment lists a child loop of depth 2
    start = next(i for i, l in enumerate(lines) if "Child Loop" in l and "Depth 2" in l)
    hdr = block_of[start]
    first = next(i for i, b in enumerate(block_of) if b == hdr)
    last = max(i for i, b in enumerate(block_of) if b is not None and depth.get(b, 0) >= 1 and i >= first)
    lab = {}
    in_probe_trip = False
    for i in range(first, last + 1):
        b, l = block_of[i], lines[i]
        d = depth.get(b, 0)
        if "=>  This Loop Header: Depth=2" in l:
            in_probe_trip = True
        if d >= 3:
            lab[i] = "walk"
        elif d == 2:
            lab[i] = "probe" if in_probe_trip else "candidate"
            if in_probe_trip and re.match(r"\s+s_cbranch", l):
                in_probe_trip = False
        else:
            lab[i] = "pose"
    return lab


def main():
    path = sys.argv[1]
    name = sys.argv[2] if len(sys.argv) > 2 else DEFAULT
    lines = kernel_lines(path, name)
    lab = regions(lines)
    keys = ["pose", "probe", "candidate", "walk"]
    tot = {k: [0, 0, 0, 0] for k in keys}   # valu, lane moves, packed, v_mul_lo
    for i, r in lab.items():
        m = re.match(r"\s+(v_\w+)", lines[i])
        if not m:
            continue
        op = m.group(1)
        tot[r][0] += 1
        tot[r][1] += op.startswith(("v_readlane", "v_writelane"))
        tot[r][2] += op.startswith("v_pk_")
        tot[r][3] += op.startswith("v_mul_lo_u32")
    print(name)
    print(f"{'region':<34}{'VALU':>6}{'readlane/writelane':>20}{'v_pk_*':>8}{'v_mul_lo_u32':>14}")
    names = {"pose": "per-pose preamble + epilogue", "probe": "probe trip (to the candidate test)",
             "candidate": "candidate block (depth 2, rest)", "walk": "walk loops (depth 3, all forms)"}
    for k in keys:
        v = tot[k]
        print(f"{names[k]:<34}{v[0]:>6}{v[1]:>20}{v[2]:>8}{v[3]:>14}")
    whole = sum(1 for l in lines if re.match(r"\s+v_\w+", l))
    print(f"{'whole kernel':<34}{whole:>6}")


if __name__ == "__main__":
    main()
