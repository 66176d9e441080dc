#!/usr/bin/env python
"""Stage timing inside tbx_front_pair (profiling build libtbx_hip_clk.so: `make -C trafficbotsv1.5_amd/csrc clk`): thread 0 of four
workgroups of the launch - the lights' first window workgroup, the agents' first window workgroup, one search workgroup (a job with
n_tgt = 1024 if there is one) and the first rider workgroup - stamps the shader clock at the stage boundaries (csrc/front.hip,
TBX_FRONT_CLK). Five single eager simulation steps; the stamps are those of each step's front launch. Only differences inside ONE
workgroup are printed: the counters of workgroups on different XCDs are not the same counter (their differences came out as 10^9), so
the clock cannot say which workgroup ends last - only how long each kind is busy. Unit: 100 shader clocks (clock64 = s_memtime = shader
clocks here, ~2.4 GHz: one unit = 0.042 us), as tools/mid_clock.py.
    python tools/front_clock.py [bench.py rollout args]"""
import ctypes as C
import os
import sys
from importlib import import_module
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ["TBX_HIP_LIB"] = str(ROOT / "trafficbotsv1.5_amd" / "csrc" / "libtbx_hip_clk.so")

import torch  # noqa: E402

import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

WIN = ["inputs requested -> in LDS", "input MLP 1", "input MLP 2", "input MLP 3", "PointNet 1", "PointNet 2", "PointNet 3 + pooled rows",
       "LayerNorm (+ units q, k requested)", "q", "k | v", "W_k^T q"]
SEARCH = ["candidates loaded", "cosf / sinf, keys, bisection", "outputs written"]
RIDER = ["inputs (pose embedding) in LDS", "stage 1", "stage 2", "stage 3", "stage 4 + store"]
SLOTS = [("lights' first window workgroup (\"add\", 128)", 0, WIN), ("agents' first window workgroup (\"cat\", 64)", 0, WIN),
         ("search workgroup", 16, SEARCH), ("rider workgroup", 20, RIDER)]
U = 100.0


def main():
    sys.argv = [sys.argv[0], "--no-cpu-baseline", "--no-graph"] + sys.argv[1:]
    args = bench.parse()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    tb = load_package()
    lib = import_module("trafficbots_amd.hip").load()
    lib.tbx_debug_front_dump.argtypes = [C.c_void_p]
    wm, full = bench.build(tb, args, dev, 0)
    eng, _ = bench.gpu_rollout_setup(tb, wm, full, args, dev)
    eng.run(args.warmup + 3, use_graph=False)
    torch.cuda.synchronize()
    buf = (C.c_uint64 * (4 * 32))()
    samples = []
    for _ in range(5):  # five single steps: stamps of five front launches
        assert lib.tbx_debug_front_dump(buf) == 0  # reset
        eng.run(1, use_graph=False)
        torch.cuda.synchronize()
        assert lib.tbx_debug_front_dump(buf) == 0
        samples.append(list(buf))
    for k, c in enumerate(samples):
        print(f"step {k} (unit: 100 shader clocks = 0.042 us)")
        for s, (name, base, stages) in enumerate(SLOTS):
            v = c[s * 32 + base:s * 32 + base + len(stages) + 1]
            if not v[0]:
                print(f"  {name}: not in this launch")
                continue
            print(f"  {name}: {(v[-1] - v[0]) / U:6.2f} inside")
            for st, a, b in zip(stages, v, v[1:]):
                print(f"      {st:40s} {(b - a) / U:6.2f}")
    # medians over the steps
    print("median over the steps (unit: 100 shader clocks = 0.042 us)")
    for s, (name, base, stages) in enumerate(SLOTS):
        if not samples[0][s * 32 + base]:
            continue
        print(f"  {name}")
        for i, st in enumerate(stages):
            d = sorted((c[s * 32 + base + i + 1] - c[s * 32 + base + i]) / U for c in samples)
            print(f"      {st:40s} {d[len(d) // 2]:6.2f}   (min {d[0]:.2f}, max {d[-1]:.2f})")
        tot = sorted((c[s * 32 + base + len(stages)] - c[s * 32 + base]) / U for c in samples)
        print(f"      {'inside (entry stamp -> last stamp)':40s} {tot[len(tot) // 2]:6.2f}")


if __name__ == "__main__":
    main()
