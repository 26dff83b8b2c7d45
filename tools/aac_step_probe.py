#!/usr/bin/env python3
"""Development tool: where the shader cycles of one step of the AAC workgroup walk go -- the wait for the prefetched lines,
barrier 1, barrier 2, everything else -- from a library built with SYMACCEL_TUNE_AAC_QUAD=2 (csrc/experiments/aac_quad_probe.h:
every wavefront leaves its running totals in the first PCM frame of its segment; the PCM is wrong by construction).
  SYMACCEL_TUNE_AAC_QUAD=2 python -m symphonia_amd.build
  SYMACCEL_LIB=symphonia_amd/build/tuned/libsymaccel.so python tools/aac_step_probe.py"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
import symphonia_amd as sa  # noqa: E402

TAG = 0x57E9C10C


def main():
    ctx = sa.Context(0)
    ctx.use_torch_stream()
    step, *_rest, pcm = bench.make_workload("aac", torch, ctx, 0)
    for _ in range(600):  # sustained: the board needs ~25 ms of load to leave its idle state, the clock then follows the load
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step()
    e1.record()
    torch.cuda.synchronize()
    words = pcm.view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1, 1024)
    print("kernel %.1f us (events)" % (e0.elapsed_time(e1) * 1e3))
    rows = []
    for wave in range(4):
        w = words[:, 16 * wave:16 * wave + 8]
        w = w[w[:, 0] == TAG]
        rows.append(w)
        if not len(w):
            continue
        pairs, b1, b2, wait, total = (w[:, i].astype(np.float64) for i in (1, 2, 3, 4, 5))
        rest = total - b1 - b2 - wait
        print("wave %d: %d walks stamped, %.0f barrier pairs each; cycles per step: total %.0f | prefetch wait %.0f | barrier 1 %.0f | barrier 2 %.0f | rest %.0f" % (
            wave, len(w), pairs.mean(), (total / pairs).mean(), (wait / pairs).mean(), (b1 / pairs).mean(), (b2 / pairs).mean(), (rest / pairs).mean()))
    allw = np.concatenate([r for r in rows if len(r)])
    if not len(allw):
        print("no stamps found: is SYMACCEL_LIB a SYMACCEL_TUNE_AAC_QUAD=2 build?")
        return 1
    pairs, b1, b2, wait, total = (allw[:, i].astype(np.float64) for i in (1, 2, 3, 4, 5))
    rest = total - b1 - b2 - wait
    per = total / pairs
    print("all wavefronts: cycles per step %.0f (min %.0f, max %.0f) = prefetch wait %.1f %% + barrier 1 %.1f %% + barrier 2 %.1f %% + rest %.1f %%" % (
        per.mean(), per.min(), per.max(), 100 * (wait / total).mean(), 100 * (b1 / total).mean(), 100 * (b2 / total).mean(), 100 * (rest / total).mean()))
    print("all wavefronts: per step: prefetch wait %.0f, barrier 1 %.0f, barrier 2 %.0f, rest %.0f shader cycles" % (
        (wait / pairs).mean(), (b1 / pairs).mean(), (b2 / pairs).mean(), (rest / pairs).mean()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
