#!/usr/bin/env python3
"""The FLAC verification kernel (symaccel_flac_md5_device) against the restore it rides on, at the batcher's operating points:
S streams, each a batch of F frames of 4096-sample 16-bit stereo (what `decoders_bench --codec flac` feeds), one wavefront per stream.

    python tools/flac_md5_time.py [--frames F] [--streams 1,16,256,1024]

Prints one JSON line per S: ms per MD5 launch, the restore of the same subframes (order-8 LPC, padded rows as the batcher lays them
out), the MD5 / restore ratio, MB/s hashed per stream and in all, and the finishing form (symaccel_flac_md5_finish_device) against
restore + MD5 + decorrelate as three launches.  Every stream's digest is checked against hashlib."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import symphonia_amd as sa  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--streams", default="1,16,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = sa.Context(0)
    ctx.use_torch_stream()
    bs, nch, nb = 4096, 2, 2
    pitch = int(ctx.lib.dll.symaccel_row_stride(bs))
    for S in [int(s) for s in a.streams.split(",")]:
        F = a.frames
        n_rows = S * F * nch
        g = torch.Generator(device="cuda").manual_seed(S)
        rows = torch.randint(-(1 << 15), 1 << 15, (n_rows, pitch), generator=g, device="cuda", dtype=torch.int32)
        frames = sa.flac_md5_frames(np.full(F, bs), np.arange(F) % 4)
        d_frames = torch.from_numpy(frames.view(np.uint8).copy()).cuda()
        states = np.repeat(sa.md5_init(ctx.lib), S)
        d_states = torch.from_numpy(states.view(np.uint8).copy()).cuda()
        d_cps = torch.zeros(S * F * sa.MD5_STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        jobs = np.zeros(S, sa.FLAC_MD5_JOB_DTYPE)
        jobs["rows"] = rows.data_ptr() + np.arange(S, dtype=np.uint64) * (F * nch * pitch * 4)
        jobs["frames"] = d_frames.data_ptr()
        jobs["state"] = d_states.data_ptr() + np.arange(S, dtype=np.uint64) * sa.MD5_STATE_DTYPE.itemsize
        jobs["checkpoints"] = d_cps.data_ptr() + np.arange(S, dtype=np.uint64) * (F * sa.MD5_STATE_DTYPE.itemsize)
        jobs["row_pitch"], jobs["n_frames"], jobs["nch"], jobs["bytes_per_sample"] = pitch, F, nch, nb
        d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
        # correctness first (one launch from the initial states), then the timing (the states run on: same work per launch)
        sa.flac_md5_device(ctx, d_jobs, S)
        torch.cuda.synchronize()
        got = d_states.cpu().numpy().view(sa.MD5_STATE_DTYPE)
        host_rows = rows[: min(S, 4) * F * nch].cpu().numpy()
        for s in range(min(S, 4)):
            r = host_rows[s * F * nch:(s + 1) * F * nch]
            data = []
            for f in range(F):
                a0, b0 = r[2 * f, :bs].astype(np.int64), r[2 * f + 1, :bs].astype(np.int64)
                m = f % 4
                if m == 1:
                    b0 = a0 - b0
                elif m == 2:
                    mid = (a0 << 1) | (b0 & 1)
                    a0, b0 = (mid + b0) >> 1, (mid - b0) >> 1
                elif m == 3:
                    a0 = a0 + b0
                data.append((np.stack([a0, b0], 1) & 0xffff).astype("<u2").tobytes())
            assert sa.md5_digest(got[s:s + 1], ctx.lib) == hashlib.md5(b"".join(data)).digest(), s
        md5_ms = timed(lambda: sa.flac_md5_device(ctx, d_jobs, S), a.reps)
        desc = torch.from_numpy(sa.flac_desc(np.full(n_rows, 2), np.full(n_rows, 8), np.full(n_rows, 11), np.zeros(n_rows)).view(np.uint8).reshape(n_rows, 4)).cuda()
        co = torch.zeros((n_rows, 32), dtype=torch.int32, device="cuda")
        co[:, :8] = torch.tensor([1500, -900, 540, -324, 194, -116, 70, -42], dtype=torch.int32)
        fp = sa.FlacPredictor(ctx)
        work = rows.clone()
        restore_ms = timed(lambda: fp.restore_strided(work, desc, co, bs), a.reps)
        # the finishing form (symaccel_flac_md5_finish_device: the MD5 walk also leaves the planes decorrelated and << 16) against what it
        # replaces on the same frames: restore + MD5 + decorrelate as three launches (the decorrelate over compact planes of the same size)
        ch0 = torch.randint(-(1 << 15), 1 << 15, (S * F, bs), generator=g, device="cuda", dtype=torch.int32)
        ch1 = ch0.clone()
        modes = torch.from_numpy((np.arange(S * F) % 4).astype(np.uint8)).cuda()
        decor_ms = timed(lambda: fp.decorrelate(modes, ch0, ch1, bs, 16), a.reps)
        finish_ms = timed(lambda: sa.flac_md5_finish_device(ctx, d_jobs, 16, S), a.reps)
        hashed = F * bs * nch * nb
        print(json.dumps({"streams": S, "frames_per_stream": F, "md5_ms": round(md5_ms, 4), "restore_ms": round(restore_ms, 4),
                          "decorrelate_ms": round(decor_ms, 4), "finish_ms": round(finish_ms, 4),
                          "restore_plus_finish_ms": round(restore_ms + finish_ms, 4), "three_launches_ms": round(restore_ms + md5_ms + decor_ms, 4),
                          "finish_path_over_three_launches": round((restore_ms + finish_ms) / (restore_ms + md5_ms + decor_ms), 3),
                          "md5_over_restore": round(md5_ms / restore_ms, 3), "us_per_block_per_stream": round(md5_ms * 1e3 / (hashed / 64), 4),
                          "MBps_per_stream": round(hashed / md5_ms / 1e3, 1), "GBps_total": round(S * hashed / md5_ms / 1e6, 2)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
