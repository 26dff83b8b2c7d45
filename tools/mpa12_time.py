#!/usr/bin/env python3
"""The fused Layer I / Layer II kernel (symaccel_mpa12_decode_pp_device: 16-bit codes + records in) against the unfused polyphase kernel
(symaccel_mpa_polyphase_pp_device: f32 sub-band samples in) on the same batch, resident in HBM.

    python tools/mpa12_time.py [--chains 128] [--packets 2048] [--reps 400] [--trials 5] [--warmup 3] [--out profiles/mpa12_decode.jsonl]

The batch: `--chains` chains x `--packets` Layer II packets, and the Layer I batch of equal bytes (three times the packets).  Every
sub-band is allocated (the most dequantisation work a packet can hold), classes / widths and scale factors at random.  The unfused
kernel gets the f32 samples tests/mpa12_ref.py makes of the first packets, tiled over the batch (what it computes does not depend on the
values).  Timed with device events: `--warmup` windows of each form first (about a second of back-to-back launches in all, so that the
board is at the clock it sustains under this load before anything is recorded), then `--trials` windows of `--reps` launches (400 launches
of ~0.6 ms: a quarter of a second per window) of one form alternating with windows of the other; medians, minima and maxima are reported.  Algorithmic bytes per sample: 2 (codes) + 4 (PCM) plus the records for the fused form,
4 + 4 for the unfused one.  The first packets of the fused form are checked against the reference arithmetic before anything is timed.
Writes one JSON line per layer to --out together with the board's clocks as rocm-smi reports them and the compiler's resource record of
both kernels (profiles/mpa12_decode.txt is the report written from them)."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import symphonia_amd as sa  # noqa: E402
import mpa12_ref as R  # noqa: E402


def window(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def resources():
    """{(n_frames, fused): the compiler's record} from the device assembly; {} without hipcc"""
    try:
        import re
        from tools.kernel_resources import device_asm, kernel_resources
        out = {}
        text = device_asm("mpa_polyphase.hip")
        for name, r in kernel_resources(text).items():
            m = re.search(r"mpa_polyphase_kernelILi(\d+)ELb(\d)E", name)
            if m:
                body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, flags=re.S | re.M).group(1)
                r = dict(r)
                r["instructions"] = {k: len(re.findall(r"^\s+%s" % p, body, flags=re.M)) for k, p in
                                     (("valu", "v_"), ("salu", "s_"), ("lds", "ds_"), ("global", "global_"), ("waitcnt", "s_waitcnt"))}
                out["nf%s_fused%s" % m.groups()] = r
        return out
    except Exception as e:  # noqa: BLE001
        print("kernel resources not read: %s" % e, file=sys.stderr)
        return {}


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout.strip().splitlines()
    except Exception as e:  # noqa: BLE001
        return ["rocm-smi not run: %s" % e]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--packets", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3, help="windows of each form run before the recorded ones")
    ap.add_argument("--no-resources", action="store_true", help="do not compile the kernels again for the resource record")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mpa12_decode.jsonl"))
    a = ap.parse_args()
    ctx = sa.Context(0)
    ctx.use_torch_stream()
    lines = [{"clocks_before": clocks()}]
    rng = np.random.default_rng(12)
    for layer in (R.LAYER2, R.LAYER1):
        nf, rb = R.N_FRAMES[layer], R.RECORD_BYTES[layer]
        nch, npk = a.chains, a.packets * (1 if layer == R.LAYER2 else 3)
        tile = 8  # packets made on the host, repeated along the packet axis
        codes = rng.integers(0, 1 << 16, (nch, tile, 32, nf)).astype(np.uint16)
        rec = np.zeros((nch, tile, rb), np.uint8)
        rec[..., :32] = rng.integers(2, 16, (nch, tile, 32)) if layer == R.LAYER1 else rng.integers(1, 18, (nch, tile, 32))
        rec[..., 32:] = rng.integers(0, 63, (nch, tile, rb - 32))
        x = R.dequantize_batch(layer, codes, rec)
        reps = (npk + tile - 1) // tile
        d_codes = torch.from_numpy(codes.view(np.int16)).cuda().repeat(1, reps, 1, 1)[:, :npk].contiguous()
        d_rec = torch.from_numpy(rec).cuda().repeat(1, reps, 1)[:, :npk].contiguous()
        d_x = torch.from_numpy(x).cuda().repeat(1, reps, 1)[:, :npk].contiguous()
        vv = [torch.zeros((nch, 1024), dtype=torch.float32, device="cuda") for _ in range(2)]
        vf = [torch.zeros(nch, dtype=torch.int32, device="cuda") for _ in range(2)]
        pcm = torch.empty((nch, npk, 32 * nf), dtype=torch.float32, device="cuda")
        pcm2 = torch.empty_like(pcm)
        dec, syn = sa.Mpa12Decode(ctx, layer), sa.MpaPolyphase(ctx, nf)

        def fused():
            dec.decode(d_codes, d_rec, vv[0], vf[0], pcm=pcm, state_out=(vv[1], vf[1]))

        def unfused():
            syn.synth(d_x, vv[0], vf[0], pcm2, state_out=(vv[1], vf[1]))

        fused()
        unfused()
        torch.cuda.synchronize()
        want = R.synthesize(layer, x[:2], np.zeros((2, 1024), np.float32), np.zeros(2, np.int32))[0]
        assert np.array_equal(pcm[:2, :tile].cpu().numpy().view(np.uint32), want.view(np.uint32)), "the fused form differs from the reference arithmetic"
        assert torch.equal(pcm.view(torch.int32), pcm2.view(torch.int32)), "fused and unfused differ"
        for _ in range(a.warmup):
            for fn in (fused, unfused):
                window(fn, a.reps)
        clocks_warm = clocks()
        t_f, t_u = [], []
        for _ in range(a.trials):
            t_f.append(window(fused, a.reps))
            t_u.append(window(unfused, a.reps))
        samples = nch * npk * 32 * nf
        b_f, b_u = samples * 6 + nch * npk * rb, samples * 8
        mf, mu = statistics.median(t_f), statistics.median(t_u)
        lines.append({"layer": layer, "chains": nch, "packets": npk, "samples": samples, "fused_ms": round(mf, 4), "fused_ms_min_max": [round(min(t_f), 4), round(max(t_f), 4)],
                      "unfused_ms": round(mu, 4), "unfused_ms_min_max": [round(min(t_u), 4), round(max(t_u), 4)], "fused_over_unfused": round(mf / mu, 4),
                      "fused_bytes": b_f, "unfused_bytes": b_u, "fused_GBps": round(b_f / mf / 1e6, 1), "unfused_GBps": round(b_u / mu / 1e6, 1),
                      "link_bytes_in_fused": samples * 2 + nch * npk * rb, "link_bytes_in_unfused": samples * 4,
                      "reps": a.reps, "trials": a.trials, "warmup_windows": a.warmup, "clocks_after_warmup": [x for x in clocks_warm if "clk" in x],
                      "clocks_after_windows": [x for x in clocks() if "clk" in x]})
        print(json.dumps(lines[-1]), flush=True)
        del d_codes, d_rec, d_x, pcm, pcm2
    lines.append({"clocks_after": clocks()})
    if not a.no_resources:
        lines.append({"resources": resources()})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in lines))
    ctx.close()


if __name__ == "__main__":
    main()
