#!/usr/bin/env python3
"""The PCM conversion kernel (symaccel_pcm_convert_device) against a plain device copy that moves the same number of bytes.

    python tools/pcm_convert_time.py [--mib 512] [--cases f32:s16:2,f32:s24:8] [--reps 200] [--trials 5]

A case is source:destination:channels.  Each converts `--mib` MiB of input planes (groups of 4096 frames at the row pitch
symaccel_row_stride() gives) and is timed with device events, `--trials` windows of `--reps` launches alternating with windows of
symaccel_probe_copy_device over (bytes read + bytes written) / 2 bytes -- the copy reads and writes that many, so both move the same
total.  Timing starts after a warm-up of the same length, at the clock the device sustains.  Prints one JSON line per case: the median
and the spread of the windows for both, the byte rates, and their ratio.  The stereo f32 -> s16 case is checked against numpy first."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import symphonia_amd as sa  # noqa: E402


def window(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=512)
    ap.add_argument("--cases", default="f32:s16:2,f32:s24:8")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--trials", type=int, default=5)
    a = ap.parse_args()
    ctx = sa.Context(0)
    ctx.use_torch_stream()
    nf = 4096
    stride = int(ctx.lib.dll.symaccel_row_stride(nf))
    for case in a.cases.split(","):
        src, dst, ch = case.split(":")
        ch = int(ch)
        b = sa.sample_bytes(dst, ctx.lib)
        groups = max(1, (a.mib << 20) // (ch * nf * 4))
        gb = nf * ch * b
        g = torch.Generator(device="cuda").manual_seed(ch)
        if src == "f32":
            planes = torch.randn((groups * ch, stride), generator=g, device="cuda", dtype=torch.float32) * 0.5
        else:
            planes = torch.randint(-(1 << 31), (1 << 31) - 1, (groups * ch, stride), generator=g, device="cuda", dtype=torch.int32)
        out = torch.zeros(groups * gb, dtype=torch.uint8, device="cuda")
        read, written = groups * ch * nf * 4, groups * gb
        copy_bytes = ((read + written) // 2 + 4095) // 4096 * 4096
        c_src = torch.zeros(copy_bytes, dtype=torch.uint8, device="cuda")
        c_dst = torch.zeros(copy_bytes, dtype=torch.uint8, device="cuda")

        def conv():
            sa.pcm_convert_device(ctx, planes, src, stride, groups, ch, nf, out, dst, gb)

        def copy():
            ctx._call(ctx.lib.dll.symaccel_probe_copy_device, c_src.data_ptr(), c_dst.data_ptr(), copy_bytes, 0, 0)

        conv()
        torch.cuda.synchronize()
        if (src, dst) == ("f32", "s16"):
            x = planes[:ch, :nf].cpu().numpy()
            want = np.trunc(np.clip(x, -1.0, 1.0) * np.float32(32768.0)).clip(-32768, 32767).astype("<i2").T.copy().view(np.uint8).ravel()
            assert np.array_equal(out[:gb].cpu().numpy(), want), "the first group differs from numpy"
        for fn in (conv, copy):  # warm-up: as long as a timed window
            window(fn, a.reps)
        t_conv, t_copy = [], []
        for _ in range(a.trials):
            t_conv.append(window(conv, a.reps))
            t_copy.append(window(copy, a.reps))
        mc, mp = statistics.median(t_conv), statistics.median(t_copy)
        rate_conv, rate_copy = (read + written) / mc / 1e6, 2 * copy_bytes / mp / 1e6
        print(json.dumps({"case": case, "groups": groups, "frames": nf, "plane_stride": stride, "MiB_read": round(read / 2**20, 1),
                          "MiB_written": round(written / 2**20, 1), "convert_ms": round(mc, 4), "convert_ms_min_max": [round(min(t_conv), 4), round(max(t_conv), 4)],
                          "copy_ms": round(mp, 4), "copy_ms_min_max": [round(min(t_copy), 4), round(max(t_copy), 4)], "convert_GBps": round(rate_conv, 1),
                          "copy_GBps": round(rate_copy, 1), "convert_over_copy": round(rate_conv / rate_copy, 3)}), flush=True)
        del planes, out, c_src, c_dst
    ctx.close()


if __name__ == "__main__":
    main()
