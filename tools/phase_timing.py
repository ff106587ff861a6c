#!/usr/bin/env python
"""Per-phase cycle breakdown of the stage-1 kernels, children_rank1_kernel or children_deep_kernel (debug build:
make -C relationalgraphlearning_amd/csrc timing; per-wave s_memtime deltas, i.e. core-clock cycles).

    RGL_HIP_LIBRARY=relationalgraphlearning_amd/lib/librgl_hip_timing.so python tools/phase_timing.py
    ... python tools/phase_timing.py prologue [roots]     the level prologue of the fused children kernel (bf16x6 searches), per level
    ... python tools/phase_timing.py stop [roots]         what the `stop` child costs in that kernel, per level: its partial tile's crowd
                                                          stage and the tile-packed head pass (RGL_FUSED_HEAD_EARLY=0: on one wave)
"""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("RGL_HIP_LIBRARY", os.path.join(ROOT, "relationalgraphlearning_amd", "lib", "librgl_hip_timing.so"))
import bench  # noqa: E402
from relationalgraphlearning_amd import _native as nat  # noqa: E402


class A:
    layers, depth, width, humans, contraction = 2, 2, 2, 19, "f32"


DEEP_NAMES = ["loop top (end barrier)", "phase A: embeddings", "barrier", "phase B: relation block / S row+col",
              "barrier + E load", "(unused)", "phase C: row scalars a, b + robot row", "per-child loop"]


PROLOGUE_NAMES = ["image + fragment loads, first barrier", "embeddings (+ fill of the wave's node rows)", "scene graph",
                  "reward / next-state pairs", "chunk barriers + closing barrier"]


def prologue_main(roots):
    """The level prologue's phases (children_fused_kernel's PRO block; counters 10..14), per wave and launch, of a depth-2 width-2
    bf16x6 search: its first level (`roots` parents, a crowd per parent) from a depth-1 search -- the same launch plan: 8 parents per
    workgroup either way at 2048 roots -- and its second level (2 x roots parents, two siblings per crowd) as depth 2 minus depth 1.
    A mark is an s_memtime round trip, ~400 cycles: two per scene, two per chunk, three per launch."""
    dev = torch.device("cuda:0")
    raw = C.CDLL(nat.LIB_PATH)
    read = raw.rgl_debug_read_fused_phase_cycles
    buf = (C.c_ulonglong * 16)()
    A.contraction = "bf16x6"
    reps, per_depth = 5, {}
    for depth in (1, 2):
        A.depth = depth
        pol = bench.make_policy(A, dev)
        ts = pol.tree_search()
        robot, humans = bench.synth_scenes(5, roots, A.humans)
        r, h = robot.to(dev), humans.to(dev)
        ts.search(r, h, roots_are_joint_states=False, want_root_values=False)
        read(buf, 1)
        for _ in range(reps):
            ts.search(r, h, roots_are_joint_states=False, want_root_values=False)
        read(buf, 1)
        per_depth[depth] = [buf[10 + i] / reps for i in range(5)]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    levels = [("level of %d parents (crowds_per 1)" % roots, per_depth[1], roots),
              ("level of %d parents (crowds_per 2)" % (2 * roots), [b - a for a, b in zip(per_depth[1], per_depth[2])], 2 * roots)]
    for name, cyc, parents in levels:
        waves = 8 * min(cus, parents)              # one 8-wave workgroup per CU
        print("%s: cycles per wave and launch" % name)
        for nm, c in zip(PROLOGUE_NAMES, cyc):
            print("  %-46s %9.0f   %5.1f %%" % (nm, c / waves, 100.0 * c / max(sum(cyc), 1)))
        print("  %-46s %9.0f" % ("total", sum(cyc) / waves))


def search_counters(roots, reps=5):
    """The fused kernel's 16 counters per search of a depth-1 and a depth-2 width-2 bf16x6 search of `roots` roots (prologue_main's
    levels: the first from depth 1, the second as the difference), and their event time in ms."""
    dev = torch.device("cuda:0")
    raw = C.CDLL(nat.LIB_PATH)
    read = raw.rgl_debug_read_fused_phase_cycles
    buf = (C.c_ulonglong * 16)()
    A.contraction = "bf16x6"
    per_depth, ms = {}, {}
    for depth in (1, 2):
        A.depth = depth
        pol = bench.make_policy(A, dev)
        ts = pol.tree_search()
        robot, humans = bench.synth_scenes(5, roots, A.humans)
        r, h = robot.to(dev), humans.to(dev)
        ts.search(r, h, roots_are_joint_states=False, want_root_values=False)
        read(buf, 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ts.search(r, h, roots_are_joint_states=False, want_root_values=False)
        e1.record()
        torch.cuda.synchronize()
        read(buf, 1)
        per_depth[depth] = [buf[i] / reps for i in range(16)]
        ms[depth] = e0.elapsed_time(e1) / reps
    return per_depth, ms


def stop_main(roots):
    """The `stop` child's two costs in the fused children kernel over a depth-1 (one launch: `roots` parents) and a depth-2 width-2
    bf16x6 search (two launches: `roots` and 2 x `roots` parents): the crowd stage of a parent's partial tile (robot row / column of
    S, softmax, p Xh, table, row pass: counter 15, per partial tile = per parent) next to a full tile's and its head, and the
    tile-packed head pass -- counter 7: what the waves that score packed tiles spend on it, per workgroup and launch; counter 0: what
    a wave spends at the loop top and waiting at the barriers behind its items (RGL_FUSED_HEAD_EARLY=0: the pass's barrier, where
    seven waves wait for the eighth's chain, and the tail's), per wave and launch.  Counter 8 is workgroup 0's clock over its
    launches.  A mark is an s_memtime round trip of ~400 cycles."""
    per_depth, ms = search_counters(roots)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("RGL_FUSED_HEAD_EARLY=%s   search: depth 1 %.4f ms, depth 2 %.4f ms (timing build)" % (
        os.environ.get("RGL_FUSED_HEAD_EARLY", "(default)"), ms[1], ms[2]))
    for depth, launches, parents in ((1, 1, roots), (2, 2, 3 * roots)):
        cyc = per_depth[depth]
        wgs = launches * min(cus, roots)
        print("depth-%d search, %d launch(es), %d parents in all: core-clock cycles" % (depth, launches, parents))
        print("  partial tile's crowd stage, per parent            %8.0f   (a full tile's: %.0f; its head: %.0f)" % (
            cyc[15] / parents, (cyc[3] + cyc[4]) / (5 * parents), cyc[6] / (5 * parents)))
        print("  tile-packed pass, per workgroup and launch        %8.0f" % (cyc[7] / wgs))
        print("  loop top + waits at the barriers, per wave, launch %7.0f" % (cyc[0] / (8 * wgs)))
        print("  workgroup 0's clock, per launch                   %8.0f" % (cyc[8] / launches))


def main():
    """usage: phase_timing.py [parents] [humans layers contraction]   (N > 32 or 3 layers -> the deep kernel's phases)"""
    if len(sys.argv) > 1 and sys.argv[1] == "prologue":
        return prologue_main(int(sys.argv[2]) if len(sys.argv) > 2 else 2048)
    if len(sys.argv) > 1 and sys.argv[1] == "stop":
        return stop_main(int(sys.argv[2]) if len(sys.argv) > 2 else 2048)
    P = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    if len(sys.argv) > 4:
        A.humans, A.layers, A.contraction = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    deep = A.layers == 3 or A.humans + 1 > 32
    dev = torch.device("cuda:0")
    pol = bench.make_policy(A, dev)
    ts = pol.tree_search()
    robot, humans = bench.synth_scenes(5, P, A.humans)
    ex = ts.expand(robot.to(dev), humans.to(dev), parents_are_joint_states=False)
    lib = nat.lib()
    raw = C.CDLL(nat.LIB_PATH)
    buf = (C.c_ulonglong * 16)()
    fused = (not deep) and os.environ.get("RGL_CHILDREN_TWO_STAGE", "0") != "1"
    read = raw.rgl_debug_read_deep_phase_cycles if deep else (raw.rgl_debug_read_fused_phase_cycles if fused
                                                              else raw.rgl_debug_read_phase_cycles)
    read(buf, 1)
    reps = 3
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ts.value_children(ex["child_robot"], ex["humans_next"])
    e1.record()
    torch.cuda.synchronize()
    read(buf, 1)
    names = DEEP_NAMES if deep else ["loop top", "embed-1 (x0, y, g0) / crowd-1 work", "mid barrier",
                                     "embed-2 (S row+col, p, pXh, a/b) / crowd-2 work", "barrier", "row phase work",
                                     "row barrier", "robot-row pass"]
    waves = 8 * P * reps          # per (wave, parent); rank-1 kernel, 8 waves per workgroup
    if fused:                     # per tile: one wave, 16 children
        names = ["loop top / value store", "tile loads issued", "embedding (x0, y, g0)", "S row+col, p, pXh, a/b", "row pass",
                 "robot row", "head", "(unused)"]
        waves = P * 6 * reps
    tot = sum(buf[i] for i in range(8))
    print("P=%d  %.3f ms per call (stage 1+2)" % (P, e0.elapsed_time(e1) / reps))
    for i, nm in enumerate(names):
        print("  %-18s %9.0f cycles per wave per parent   %5.1f %%" % (nm, buf[i] / waves, 100.0 * buf[i] / tot))
    print("  total              %9.0f" % (tot / waves))
    if buf[9]:
        print("  s_memtime / s_memrealtime (100 MHz) over the kernel: %.1f -> counter clock %.0f MHz" % (buf[8] / buf[9], 100.0 * buf[8] / buf[9]))


if __name__ == "__main__":
    main()
