#!/usr/bin/env python3
"""The PCM / G.711 decode kernel (symaccel_pcm_decode_device), resident, against two yardsticks on the same board in the same run: a plain
device copy of the same in + out bytes, and symaccel_pcm_convert_device (F32 planes in) writing the same output bytes.

    python tools/pcm_time.py [--mib 2048] [--window-ms 250] [--trials 5] [--out profiles/pcm_decode.jsonl] [--report profiles/pcm_decode.txt]

Five forms: s16le stereo -> native, s24be stereo -> f32, mu-law mono -> f32, f32le 8 channels -> native, s24le 3 channels at an odd base
offset -> s16; each as ONE packet of about `--mib` MiB of output plus input (a tile is a frame range of a packet, so one packet fills
the device; the default is eight times the 256 MiB last-level cache, below which the figures are the cache's and exceed the HBM peak).  A form is timed with device events: after a warm-up window, `--trials` windows of about `--window-ms` each, the three
kernels alternating window by window; the median is reported with the spread.  Rates are bytes read + bytes written per second of one
launch.  The first frames of every form are checked against tests/pcm_decode_ref.py before anything is timed.  The host-to-host rate of
symaccel_pcm_decode (pageable numpy memory in and out) is reported for the first form.  Nothing here is a pass or fail."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import symphonia_amd as sa  # noqa: E402
import pcm_decode_ref as R  # noqa: E402

PEAK_GBPS = 8000.0
# name, codec, channels, output format (0 = native), source offset
FORMS = (("s16le stereo -> native", "s16le", 2, 0, 0), ("s24be stereo -> f32", "s24be", 2, "f32", 0), ("mulaw mono -> f32", "mulaw", 1, "f32", 0),
         ("f32le 8ch -> native", "f32le", 8, 0, 0), ("s24le 3ch odd base -> s16", "s24le", 3, "s16", 1))


def window(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def reps_for(fn, window_ms):
    return max(3, int(window_ms / max(window(fn, 3), 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=2048)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pcm_decode.jsonl"))
    ap.add_argument("--report", default=str(ROOT / "profiles" / "pcm_decode.txt"))
    a = ap.parse_args()
    ctx = sa.Context(0)
    ctx.use_torch_stream()
    lines = []
    for name, codec, ch, fmt, s_off in FORMS:
        cb = R.coded_bytes(codec)
        ob = R.native_bytes(codec) if fmt == 0 else R.DEST_BYTES[fmt]
        frames = (a.mib << 20) // (ch * (cb + ob)) // 64 * 64
        read, written = frames * ch * cb, frames * ch * ob
        g = torch.Generator(device="cuda").manual_seed(cb * 16 + ch)
        src = torch.randint(0, 256, (read + 16,), generator=g, device="cuda", dtype=torch.uint8)
        out = torch.zeros(written, dtype=torch.uint8, device="cuda")
        copy_bytes = ((read + written) // 2 + 4095) // 4096 * 4096
        c_src = torch.zeros(copy_bytes, dtype=torch.uint8, device="cuda")
        c_dst = torch.zeros(copy_bytes, dtype=torch.uint8, device="cuda")
        planes = torch.zeros(ch * frames, dtype=torch.float32, device="cuda")  # the conversion kernel's input: F32 planes
        conv_fmt = fmt if fmt != 0 else {1: "u8", 2: "s16", 4: "f32"}[ob]
        conv_out = torch.zeros(written, dtype=torch.uint8, device="cuda")

        def decode():
            sa.pcm_decode_device(ctx, src.data_ptr() + s_off, read, 1, codec, ch, 0, frames, out, fmt)

        def copy():
            ctx._call(ctx.lib.dll.symaccel_probe_copy_device, c_src.data_ptr(), c_dst.data_ptr(), copy_bytes, 0, 0)

        def convert():
            sa.pcm_convert_device(ctx, planes, "f32", frames, 1, ch, frames, conv_out, conv_fmt, written)

        decode()
        torch.cuda.synchronize()
        k = 1000
        head = src[s_off:s_off + k * ch * cb].cpu().numpy()[None, :]
        want = R.decode(head, codec, ch, k)
        if fmt == 0:
            got = out.cpu().numpy().reshape(ch, frames * ob)[:, :k * ob]
            assert np.array_equal(got.ravel(), want.view(np.uint8).ravel()), "the first frames differ from the restatement"
        else:
            assert np.array_equal(out[:k * ch * ob].cpu().numpy(), R.interleave(want, R.CODECS[codec][3], fmt).ravel()), "the first frames differ from the restatement"
        fns = {"decode": decode, "copy": copy, "convert": convert}
        reps = {n: reps_for(f, a.window_ms) for n, f in fns.items()}  # (also the warm-up)
        for n, f in fns.items():
            window(f, reps[n])
        t = {n: [] for n in fns}
        for _ in range(a.trials):
            for n, f in fns.items():
                t[n].append(window(f, reps[n]))
        md, mc, mv = (statistics.median(t[n]) for n in ("decode", "copy", "convert"))
        rate, rate_copy, rate_conv = (read + written) / md / 1e6, 2 * copy_bytes / mc / 1e6, (frames * ch * 4 + written) / mv / 1e6
        line = {"form": name, "frames": frames, "MiB_read": round(read / 2**20, 1), "MiB_written": round(written / 2**20, 1), "decode_ms": round(md, 4),
                "decode_ms_min_max": [round(min(t["decode"]), 4), round(max(t["decode"]), 4)], "decode_GBps": round(rate, 1), "of_8TBps_peak": round(rate / PEAK_GBPS, 4),
                "copy_ms": round(mc, 4), "copy_GBps": round(rate_copy, 1), "convert_form": "f32 planes -> %s" % conv_fmt, "convert_ms": round(mv, 4),
                "convert_GBps": round(rate_conv, 1), "decode_over_copy": round(rate / rate_copy, 4), "decode_over_convert": round(rate / rate_conv, 4),
                "reps_per_window": reps}
        if name == FORMS[0][0]:  # host to host, pageable memory both ways
            h = src[:read].cpu().numpy()[None, :]
            sa.pcm_decode(ctx, h, codec, ch, frames)
            t0 = time.perf_counter()
            sa.pcm_decode(ctx, h, codec, ch, frames)
            dt = time.perf_counter() - t0
            line["host_to_host_GBps"] = round((read + written) / dt / 1e9, 2)
        lines.append(line)
        print(json.dumps(line), flush=True)
        del src, out, c_src, c_dst, planes, conv_out
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in lines))
    rep = ["symaccel_pcm_decode_device, one packet of %d MiB in + out per form, one MI355X; medians of %d windows of ~%d ms, kernels alternating" % (a.mib, a.trials, a.window_ms),
           "(tools/pcm_time.py; rates are bytes read + written per second of a launch; copy = symaccel_probe_copy_device over the same total;",
           " convert = symaccel_pcm_convert_device from F32 planes writing the same output bytes)", "",
           "%-28s %10s %10s %10s %8s %8s" % ("form", "decode", "copy", "convert", "/copy", "/convert")]
    for x in lines:
        rep.append("%-28s %8.0f GB/s %6.0f GB/s %6.0f GB/s %8.2f %8.2f" % (x["form"], x["decode_GBps"], x["copy_GBps"], x["convert_GBps"], x["decode_over_copy"], x["decode_over_convert"]))
    if "host_to_host_GBps" in lines[0]:
        rep += ["", "host to host (symaccel_pcm_decode, pageable memory), %s: %.2f GB/s in + out" % (lines[0]["form"], lines[0]["host_to_host_GBps"])]
    Path(a.report).write_text("\n".join(rep) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
