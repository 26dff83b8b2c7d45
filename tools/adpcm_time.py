#!/usr/bin/env python3
"""The ADPCM decode kernel (symaccel_adpcm_decode_device), resident, against a plain device copy that moves the same number of bytes and
against a 16-thread host restatement.

    python tools/adpcm_time.py [--tiles 5120] [--reps 20] [--trials 5] [--out profiles/adpcm_decode.jsonl]

Three cases -- MS stereo in 1024-byte blocks, IMA WAV mono in 512-byte blocks, IMA QT stereo (68-byte blocks) -- each with the native
planes (left-justified i32) and with S16 as the output, at a batch of `--tiles` 64-block tiles per 1024 bytes of block (twice what the
grid holds at once for the large blocks, more for the small ones).  A case is timed with device events, `--trials` windows of `--reps`
launches alternating with windows of symaccel_probe_copy_device over (bytes read + bytes written) / 2 bytes -- the copy reads and writes
that many, so both move the same total -- after a warm-up of the same length.  The host figure is the numpy restatement of
tests/adpcm_ref.py (vectorised across blocks) on 16 threads over a part of the batch, scaled to the whole.  There is no parent-commit
number for a new codec: the ratio to the copy and the restatement's time are reported, neither is a pass or fail (the restatement is numpy driven from a
Python thread pool, no tuned decoder: no speed-up is derived from it).  The first tile of every case is
checked against the restatement before anything is timed.  Writes one JSON line per case and output format to --out (profiles/adpcm_decode.txt is the report written from them)."""
import argparse
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import symphonia_amd as sa  # noqa: E402
import adpcm_ref as R  # noqa: E402

PEAK_GBPS = 8000.0
CASES = (("ms", 2, 1012), ("ima_wav", 1, 1017), ("ima_qt", 2, 64))


def window(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def resources():
    """{(codec, channels, sample bytes): (VGPRs, LDS bytes)} from the device assembly; {} without hipcc"""
    try:
        import re
        from tools.kernel_resources import device_asm, kernel_resources
        out = {}
        for name, r in kernel_resources(device_asm("adpcm.hip")).items():
            m = re.search(r"adpcm_decode_kernelILi(\d)ELj(\d)ELj(\d)E", name)
            if m:
                out[tuple(int(x) for x in m.groups())] = (r.get("NumVgprs"), r.get("LDSByteSize"))
        return out
    except Exception as e:  # noqa: BLE001  (no compiler on this machine: the figures are in tests/test_adpcm_build.py's output)
        print("kernel resources not read: %s" % e, file=sys.stderr)
        return {}


def host_ms_per_block(blocks, codec, ch, fpb, threads=16):
    parts = np.array_split(blocks, threads)
    with ThreadPoolExecutor(threads) as ex:
        t = time.perf_counter()
        list(ex.map(lambda p: R.decode(p, codec, ch, fpb), parts))
        return (time.perf_counter() - t) * 1e3 / len(blocks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=5120)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--host-blocks", type=int, default=4096)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "adpcm_decode.jsonl"))
    a = ap.parse_args()
    ctx = sa.Context(0)
    ctx.use_torch_stream()
    res = resources()
    lines = []
    for codec, ch, fpb in CASES:
        nb = sa.adpcm_block_bytes(codec, ch, fpb, ctx.lib)
        n = 64 * a.tiles * max(1, 1024 // nb)
        g = torch.Generator(device="cuda").manual_seed(nb)
        src = torch.randint(0, 256, (n, nb), generator=g, device="cuda", dtype=torch.uint8)
        if codec == "ms":
            src[:, :ch] %= 7
        elif codec == "ima_wav":
            src[:, 2] %= 89
        status = torch.zeros(n, dtype=torch.uint8, device="cuda")
        host = src[:a.host_blocks].cpu().numpy()
        want, _ = R.decode(host[:64], codec, ch, fpb)
        host_ms = host_ms_per_block(host, codec, ch, fpb) * n
        for fmt in (0, "s16"):
            sb = 4 if fmt == 0 else 2
            out = torch.zeros(n * ch * fpb * sb, dtype=torch.uint8, device="cuda")
            read, written = n * nb, n * ch * fpb * sb
            copy_bytes = ((read + written) // 2 + 4095) // 4096 * 4096
            c_src = torch.zeros(copy_bytes, dtype=torch.uint8, device="cuda")
            c_dst = torch.zeros(copy_bytes, dtype=torch.uint8, device="cuda")

            def decode():
                sa.adpcm_decode_device(ctx, src, nb, n, codec, ch, fpb, out, fmt, status)

            def copy():
                ctx._call(ctx.lib.dll.symaccel_probe_copy_device, c_src.data_ptr(), c_dst.data_ptr(), copy_bytes, 0, 0)

            decode()
            torch.cuda.synchronize()
            first = out[:64 * ch * fpb * sb].cpu().numpy()
            if fmt == 0:
                assert np.array_equal(first.view(np.int32).reshape(64, ch, fpb), want), "the first tile differs from the restatement"
            else:
                assert np.array_equal(first.view(np.int16).reshape(64, fpb, ch), (want >> 16).astype(np.int16).transpose(0, 2, 1)), "the first tile differs (s16)"
            for fn in (decode, copy):
                window(fn, a.reps)
            t_dec, t_copy = [], []
            for _ in range(a.trials):
                t_dec.append(window(decode, a.reps))
                t_copy.append(window(copy, a.reps))
            md, mc = statistics.median(t_dec), statistics.median(t_copy)
            rate, rate_copy = (read + written) / md / 1e6, 2 * copy_bytes / mc / 1e6
            vgpr, lds = res.get(({"ms": 1, "ima_wav": 2, "ima_qt": 3}[codec], ch, 0 if fmt == 0 else 2), (None, None))
            lines.append({"case": "%s ch%d %d-byte blocks" % (codec, ch, nb), "out": "native i32" if fmt == 0 else "s16", "blocks": n,
                          "MiB_read": round(read / 2**20, 1), "MiB_written": round(written / 2**20, 1), "decode_ms": round(md, 4),
                          "decode_ms_min_max": [round(min(t_dec), 4), round(max(t_dec), 4)], "decode_GBps": round(rate, 1),
                          "of_8TBps_peak": round(rate / PEAK_GBPS, 4), "Msamples_per_s": round(n * ch * fpb / md / 1e3, 1), "copy_ms": round(mc, 4),
                          "copy_GBps": round(rate_copy, 1), "decode_over_copy": round(rate / rate_copy, 4), "numpy_restatement_16_threads_ms": round(host_ms, 1), "VGPRs": vgpr, "LDS_bytes": lds})
            print(json.dumps(lines[-1]), flush=True)
            del out, c_src, c_dst
        del src, status
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in lines))
    ctx.close()


if __name__ == "__main__":
    main()
