"""The batcher's converting scatter (symaccel_batcher_reserve_fmt / _submit_fmt): a ticket's PCM delivered as interleaved samples of the
caller's format, converted on the way out of the device.

For each of the eight kinds ONE group holds five tickets -- the native planes, S16 interleaved, S24 planar, U8 and F32 interleaved -- and
each equals the numpy conversion (tests/test_pcm_convert.py: the restatement that is checked against the reference's conv.rs) of what the
SAME submission returns without a format from a batcher of its own.  Also checked: slot.out_bytes at reserve() and after wait(), launches
and chunks equal to the run without formats, the state planes, the Vorbis valid prefix (a first block after a reset included) and the
ticket whose chains of one interleave group disagree, and that collect() writes nothing beyond out_bytes.  CPU emulation here, gpu-marked
twins on the MI355X; `-m sanitize` runs this file against the emulation build whose host C++ is compiled under ASan + UBSan."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from emu_lib import emu_ctx  # noqa: F401
from symphonia_amd import (AAC_JS_DTYPE, AAC_TNS_DTYPE, BATCH_AAC_DECODE, BATCH_AAC_SYNTH, BATCH_ALAC_PREDICT, BATCH_FLAC_RESTORE, BATCH_MP3_DECODE,
                           BATCH_MP3_SYNTH, BATCH_VORBIS_DECODE, BATCH_VORBIS_SYNTH, Batcher, Context, SymaccelError, alac_desc, flac_desc, mp3_side)
from test_pcm_convert import BYTES, expected

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
GUARD = 0x5A


def ticket_formats(channels):
    """the five tickets of a group: native, S16 interleaved, S24 planar, U8 and F32 interleaved"""
    return [(None, 0), ("s16", channels), ("s24", 1), ("u8", channels), ("f32", channels)]


# ---- one submission per kind: (kind, param, n_chains, units, input planes, state planes, source format, interleave channels) ----------

def sub_aac_synth(b, i):
    from test_staging import aac_case
    coeffs, side, delay = aac_case(2, 3, 800 + i)
    return dict(kind=BATCH_AAC_SYNTH, param=0, n_chains=2, units=3, ins=[coeffs, side], states=[delay], src="f32", channels=2)


def sub_mp3_synth(b, i):
    from test_batcher import mp3_streams
    xr, side, ov, vv, vf, _ = mp3_streams(np.random.default_rng(810 + i), 2, 4)[1]  # (the stereo one)
    return dict(kind=BATCH_MP3_SYNTH, param=2, n_chains=2, units=4, ins=[xr, side], states=[ov, vv, vf], src="f32", channels=2)


def sub_mp3_decode(b, i):
    from test_mp3_stereo import fused_case, side_of
    q, rd, pairs, sd, _, _ = fused_case(820 + i, 1, 1, 4)
    side = side_of(rd, pairs, sd)
    chains = [int(pairs[0][0]), int(pairs[0][1])]
    rng = np.random.default_rng(830 + i)
    ov, vv, vf = rng.standard_normal((2, 576)).astype(F), rng.standard_normal((2, 1024)).astype(F), rng.integers(0, 16, 2).astype(np.int32)
    return dict(kind=BATCH_MP3_DECODE, param=1, n_chains=2, units=4, states=[ov, vv, vf], src="f32", channels=2,
                ins=[np.ascontiguousarray(q[chains]), np.ascontiguousarray(rd[chains]), np.ascontiguousarray(side[chains]), np.ascontiguousarray(sd[0])])


def vorbis_counts(flags, prev, e0, e1):
    """(first sample the chain's blocks write, samples its flags account for): lib.rs:298-303 -- a first block after a reset keeps
    n / 2 slots that nothing writes"""
    bs = (1 << e0, 1 << e1)
    p, s, first = (-1 if prev < 0 else int(prev != 0)), 0, 0
    for k, f in enumerate(flags):
        f = int(f != 0)
        s += (bs[p] + bs[f]) // 4 if p >= 0 else bs[f] // 2
        if k == 0 and p < 0:
            first = bs[f] // 2
        p = f
    return first, s


def sub_vorbis_synth(b, i, nb=6, e0=8, e1=11, mismatch=False):
    """two chains with the SAME flags and previous flag (one interleave group must agree in its sample count); stream 0 starts after a
    reset, so its first block yields nothing"""
    rng = np.random.default_rng(840 + i)
    flags = (rng.random(nb) < 0.5).astype(np.uint8)
    prev = np.int32(-1 if i % 2 == 0 else int(rng.integers(0, 2)))
    cap = nb << (e1 - 1)
    spec = (rng.standard_normal((2, cap)) * 0.25).astype(F)
    fl = np.stack([flags, flags])
    if mismatch:
        fl[1, nb // 2] ^= 1
    return dict(kind=BATCH_VORBIS_SYNTH, param=e0 | (e1 << 8), n_chains=2, units=nb, ins=[spec, np.ascontiguousarray(fl)],
                states=[np.array([prev, prev], np.int32), rng.standard_normal((2, (1 << e1) // 2)).astype(F)], src="f32", channels=2,
                vorbis=[vorbis_counts(fl[c], prev, e0, e1) for c in range(2)])


def sub_aac_decode(b, i):
    """the blob of include/symaccel.h: { n_pairs, n_tns, 0, 0 }, pair_chains padded to 16 bytes, the joint-stereo rows padded to 16 bytes, the filters"""
    import test_aac_tools as T
    from test_aac_js_fused import decode_case
    frames = 3
    coeffs, side, delay, pairs, desc, filt, _, _ = decode_case(850 + i, 1, 0, frames, 0.5)
    bands = b.aac_bands(T.SWB_LONG, T.SWB_SHORT)
    pad16 = lambda x: x + b"\0" * (-len(x) % 16)  # noqa: E731
    filt = np.ascontiguousarray(filt, AAC_TNS_DTYPE) if len(filt) else np.zeros(0, AAC_TNS_DTYPE)
    blob = np.array([1, len(filt), 0, 0], np.uint32).tobytes() + pad16(np.ascontiguousarray(pairs, np.int32).tobytes()) + \
        pad16(np.ascontiguousarray(desc, AAC_JS_DTYPE).tobytes()) + filt.tobytes()
    return dict(kind=BATCH_AAC_DECODE, param=bands, n_chains=2, units=frames, ins=[coeffs, side, np.frombuffer(blob, np.uint8)], states=[delay], src="f32",
                channels=2)


def sub_vorbis_decode(b, i, nb=5, e0=8, e1=11):
    from test_batcher_kinds import vorbis_stream
    s = vorbis_stream(b, 4300 + i, e0, e1, 2, nb)
    first = np.ascontiguousarray(s["first"], np.uint32).tobytes()
    blob = first + b"\0" * (-len(first) % 16) + np.ascontiguousarray(s["coupling"], np.uint8).tobytes()
    return dict(kind=BATCH_VORBIS_DECODE, param=e0 | (e1 << 8) | (2 << 16), n_chains=2, units=nb, src="f32", channels=2,
                ins=[s["res"], s["flags"], s["floor"], s["posts"], np.frombuffer(blob, np.uint8)], states=[s["prev0"].copy(), s["overlap"]],
                vorbis=[vorbis_counts(s["flags"][c], s["prev0"][c], e0, e1) for c in range(2)])


def sub_flac(b, i, blocksize=100):
    from test_batcher_kinds import flac_stream
    nch = 2
    buf, kind, order, shift, wasted, coeffs = flac_stream(np.random.default_rng(860 + i), 3, nch, blocksize)
    buf = (buf.astype(np.int64) << 8).astype(np.int32) if i % 2 else buf  # (samples that reach the top bits, as after `<< (32 - bps)`)
    return dict(kind=BATCH_FLAC_RESTORE, param=0, n_chains=buf.shape[0], units=blocksize, states=[], src="s32", channels=nch,
                ins=[buf, np.ascontiguousarray(flac_desc(kind, order, shift, wasted)), coeffs])


def sub_flac_padded_rows(b, i):
    return sub_flac(b, i, 1024)  # (the device plane's rows at symaccel_row_stride(1024) = 1152 words)


def sub_alac(b, i, blocksize=100):
    from test_batcher_kinds import alac_stream
    buf, mode, order, shift, bps, coeffs = alac_stream(np.random.default_rng(870 + i), 6, blocksize)
    return dict(kind=BATCH_ALAC_PREDICT, param=0, n_chains=6, units=blocksize, states=[], src="s32", channels=2,
                ins=[buf, np.ascontiguousarray(alac_desc(mode, order, shift, bps)), coeffs])


KINDS = {"aac_synth": sub_aac_synth, "mp3_synth": sub_mp3_synth, "mp3_decode": sub_mp3_decode, "vorbis_synth": sub_vorbis_synth, "aac_decode": sub_aac_decode,
         "vorbis_decode": sub_vorbis_decode, "flac_restore": sub_flac, "flac_restore_padded_rows": sub_flac_padded_rows, "alac_predict": sub_alac}
COPY_FORM = [k for k in KINDS if k not in ("aac_decode", "vorbis_decode")]  # (those two have typed submit calls that build their blobs)


# ---- running a group -----------------------------------------------------------------------------------------------------------------

def view(ptr, n):
    return np.frombuffer((C.c_char * n).from_address(ptr), np.uint8) if n else np.zeros(0, np.uint8)


def native_bytes(s):
    k = s["kind"]
    if k in (BATCH_AAC_SYNTH, BATCH_AAC_DECODE):
        per_unit = 1024
    elif k in (BATCH_MP3_SYNTH, BATCH_MP3_DECODE):
        per_unit = 576
    elif k in (BATCH_VORBIS_SYNTH, BATCH_VORBIS_DECODE):
        per_unit = 1 << (((s["param"] >> 8) & 255) - 1)
    else:
        per_unit = 1
    return s["n_chains"] * s["units"] * per_unit * 4


def run_group(ctx, make, formats, n=5):
    """n submissions of one kind through a batcher of their own, zero-copy form, ticket i with formats[i]; returns per ticket the valid
    output bytes, out_bytes at reserve() and after wait(), the state planes, the status, and the batcher's statistics"""
    b = Batcher(ctx, 0)
    subs = [make(b, i) for i in range(n)]
    live = []
    for s, (fmt, ch) in zip(subs, formats):
        t, slot = b.reserve(s["kind"], s["param"], s["n_chains"], s["units"], out_format=fmt or 0, channels=ch)
        for k, a in enumerate(s["ins"]):
            dst = view(slot.input[k], slot.input_bytes[k])
            dst[:] = 0
            src = np.ascontiguousarray(a).view(np.uint8).ravel()
            assert len(src) <= len(dst), (k, len(src), len(dst))
            dst[:len(src)] = src
        for k, a in enumerate(s["states"]):
            view(slot.state[k], slot.state_bytes[k])[:] = np.ascontiguousarray(a).view(np.uint8).ravel()
        live.append((t, int(slot.out_bytes), [(int(slot.state[k]), int(slot.state_bytes[k])) for k in range(len(s["states"]))]))
        b.commit(t)
    res = []
    for (t, reserved, state_at), s in zip(live, subs):
        try:
            slot = b.wait(t)
            out = view(slot.out, slot.out_bytes).copy()
            states = [view(slot.state[k], slot.state_bytes[k]).copy() for k in range(len(s["states"]))]
            res.append(dict(status=0, out=out, reserved=reserved, states=states))
        except SymaccelError as e:
            # (wait() gives the same pointers reserve() gave: what a failed submission left in its state planes)
            res.append(dict(status=e.status, out=None, reserved=reserved, states=[view(p, n).copy() for p, n in state_at]))
        b.release(t)
    st = b.stats()
    b.close()
    return subs, res, st


def want_bytes(s, native, fmt, ch):
    """the conversion of the native planes, and a mask of the bytes the launch defines (Vorbis: not the slots in front of a first block)"""
    planes = native.view(np.float32 if s["src"] == "f32" else np.int32).reshape(s["n_chains"], -1)
    b = BYTES[fmt]
    if "vorbis" not in s:
        w = expected(s["src"], fmt, planes, ch, planes.shape[1]).ravel()
        return w, np.ones(len(w), bool)
    outs, masks = [], []
    for c in range(0, s["n_chains"], ch):
        first, count = s["vorbis"][c]
        w = expected(s["src"], fmt, planes[c:c + ch], ch, count).ravel()
        m = np.ones(len(w), bool)
        m[:first * ch * b] = False
        outs.append(w)
        masks.append(m)
    return np.concatenate(outs), np.concatenate(masks)


def check_kind(ctx, name):
    make = KINDS[name]
    subs, base, st0 = run_group(ctx, make, [(None, 0)] * 5)
    assert all(r["status"] == 0 for r in base) and st0["launches"] == 1 and st0["failed_tickets"] == 0, st0
    channels = subs[0]["channels"]
    formats = ticket_formats(channels)
    subs, got, st1 = run_group(ctx, make, formats)
    assert (st1["launches"], st1["chunks"], st1["submissions"], st1["failed_tickets"]) == (st0["launches"], st0["chunks"], 5, 0), (st0, st1)
    for i, (s, (fmt, ch), r0, r1) in enumerate(zip(subs, formats, base, got)):
        assert r1["status"] == 0, (name, i)
        assert len(r0["out"]) == native_bytes(s)
        for a, bb in zip(r0["states"], r1["states"]):
            assert np.array_equal(a, bb), (name, i, "state planes are never converted")
        if fmt is None:
            assert r1["reserved"] == native_bytes(s) and len(r1["out"]) == native_bytes(s)
            if "vorbis" not in s:
                assert np.array_equal(r1["out"], r0["out"]), (name, i)
            continue
        want, defined = want_bytes(s, r0["out"], fmt, ch)
        assert r1["reserved"] == native_bytes(s) // 4 * BYTES[fmt], (name, i, "out_bytes at reserve(): the most the shape can give")
        assert len(r1["out"]) == len(want), (name, i, fmt, len(r1["out"]), len(want))
        bad = np.flatnonzero((r1["out"] != want) & defined)
        assert bad.size == 0, "%s ticket %d (%s x %d): %d bytes differ, first at %d" % (name, i, fmt, ch, bad.size, bad[0])
    return st0, st1


@pytest.mark.parametrize("name", list(KINDS))
def test_emu_every_kind_converts_in_the_scatter(emu_ctx, name):
    check_kind(emu_ctx, name)


def check_copy_form(ctx, name):
    """submit_fmt / collect: exactly out_bytes bytes reach the caller's buffer"""
    make = KINDS[name]
    subs, base, _ = run_group(ctx, make, [(None, 0)] * 5)
    b = Batcher(ctx, 0)
    subs = [make(b, i) for i in range(5)]
    formats = ticket_formats(subs[0]["channels"])
    outs, tickets, states = [], [], []
    for s, (fmt, ch) in zip(subs, formats):
        out = np.full(native_bytes(s) + 64, GUARD, np.uint8)
        st = [np.ascontiguousarray(a).copy() for a in s["states"]]
        tickets.append(b.submit(s["kind"], s["param"], [np.ascontiguousarray(a) for a in s["ins"]], st, out, out_format=fmt or 0, channels=ch,
                                n_chains=s["n_chains"], units=s["units"]))
        outs.append(out)
        states.append(st)
    for t in reversed(tickets):
        b.collect(t)
    assert b.stats()["launches"] == 1
    b.close()
    for i, (s, (fmt, ch), r0, out, st) in enumerate(zip(subs, formats, base, outs, states)):
        for a, bb in zip(r0["states"], st):
            assert np.array_equal(a, bb.view(np.uint8).ravel()), (name, i)
        if fmt is None:
            n, want, defined = native_bytes(s), r0["out"], np.ones(native_bytes(s), bool)
            if "vorbis" in s:
                continue
        else:
            want, defined = want_bytes(s, r0["out"], fmt, ch)
            n = len(want)
        assert np.array_equal(out[:n][defined], want[defined]), (name, i, fmt)
        assert np.all(out[n:] == GUARD), "%s ticket %d: collect() wrote beyond out_bytes" % (name, i)


@pytest.mark.parametrize("name", COPY_FORM)
def test_emu_collect_writes_exactly_out_bytes(emu_ctx, name):
    check_copy_form(emu_ctx, name)


def check_vorbis_mismatch(ctx):
    """chains of one interleave group whose flags account for different sample counts: that ticket fails alone"""
    def make(b, i):
        return sub_vorbis_synth(b, i, mismatch=(i == 2))
    formats = [("s16", 2), (None, 0), ("s16", 2), ("s16", 1), ("u8", 2)]
    subs, base, st0 = run_group(ctx, make, [(None, 0)] * 5)
    subs, got, st = run_group(ctx, make, formats)
    assert [r["status"] for r in got] == [0, 0, -1, 0, 0] and st["failed_tickets"] == 1 and st["launches"] == 1, st
    for i in (0, 3, 4):
        fmt, ch = formats[i]
        s = dict(subs[i])
        want, defined = want_bytes(s, base[i]["out"], fmt, ch)
        assert len(got[i]["out"]) == len(want) and np.array_equal(got[i]["out"][defined], want[defined]), i
    # the failed one ran as an empty description: its state planes are those of the same flags over silence
    def make_silent(b, i):
        s = make(b, i)
        if i == 2:
            s["ins"][0] = np.zeros_like(s["ins"][0])
        return s
    _, silent, _ = run_group(ctx, make_silent, [(None, 0)] * 5)
    for a, bb in zip(got[2]["states"], silent[2]["states"]):
        assert np.array_equal(a, bb), "the failed submission did not run as silence"
    assert not np.array_equal(base[2]["states"][1], silent[2]["states"][1])  # (the case can tell the two apart)
    # the same chains as two groups of one channel each are fine: every chain has its own count
    formats[2] = ("s16", 1)
    subs, got, st = run_group(ctx, make, formats)
    assert [r["status"] for r in got] == [0] * 5 and st["failed_tickets"] == 0
    want, defined = want_bytes(subs[2], base[2]["out"], "s16", 1)
    assert len(got[2]["out"]) == len(want) and np.array_equal(got[2]["out"][defined], want[defined])


def test_emu_vorbis_group_that_disagrees_fails_alone(emu_ctx):
    check_vorbis_mismatch(emu_ctx)


def check_vorbis_first_block(ctx):
    """a batch that starts after a reset: the first block's n / 2 slots are counted (lib.rs:303) and nothing defined is in them -- with
    one block that is all there is (only the count can be checked); with two, the second block's samples follow them"""
    for nb in (1, 2):
        def make(b, i):
            s = sub_vorbis_synth(b, 2 * i, nb=nb)
            assert s["vorbis"][0][0] > 0 and (nb > 1 or s["vorbis"][0][0] == s["vorbis"][0][1])
            return s
        _, base, _ = run_group(ctx, make, [(None, 0)] * 5)
        subs, got, st = run_group(ctx, make, ticket_formats(2))
        for s, (fmt, ch), r0, r in zip(subs, ticket_formats(2), base, got):
            assert r["status"] == 0
            if fmt:
                want, defined = want_bytes(s, r0["out"], fmt, ch)
                assert len(r["out"]) == s["vorbis"][0][1] * 2 * BYTES[fmt] == len(want)
                assert defined.any() == (nb > 1) and np.array_equal(r["out"][defined], want[defined]), (nb, fmt)


def test_emu_vorbis_first_block_after_a_reset_yields_nothing(emu_ctx):
    check_vorbis_first_block(emu_ctx)


def check_reserve_fmt_refusals(ctx):
    b = Batcher(ctx, 0)
    for fmt, ch, n in ((10, 2, 2), (-1, 1, 2), ("s16", 0, 2), ("s16", 9, 18), ("s16", 2, 3), ("s24", 4, 6)):
        with pytest.raises(SymaccelError) as e:
            b.reserve(BATCH_AAC_SYNTH, 0, n, 2, out_format=fmt, channels=ch)
        assert e.value.status == -1
    t, slot = b.reserve(BATCH_AAC_SYNTH, 0, 6, 2, out_format="s24", channels=3)
    assert slot.out_bytes == 6 * 2 * 1024 * 3
    b.release(t)
    assert b.stats()["pending"] == 0
    b.close()


def test_emu_what_reserve_fmt_refuses(emu_ctx):
    check_reserve_fmt_refusals(emu_ctx)


# ---- the MI355X ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on an MI355X (there is no CPU path)")
    ctx = Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KINDS))
def test_gpu_every_kind_converts_in_the_scatter(gpu_ctx, name):
    check_kind(gpu_ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", COPY_FORM)
def test_gpu_collect_writes_exactly_out_bytes(gpu_ctx, name):
    check_copy_form(gpu_ctx, name)


@pytest.mark.gpu
def test_gpu_vorbis_group_that_disagrees_fails_alone(gpu_ctx):
    check_vorbis_mismatch(gpu_ctx)


@pytest.mark.gpu
def test_gpu_vorbis_first_block_after_a_reset_yields_nothing(gpu_ctx):
    check_vorbis_first_block(gpu_ctx)


@pytest.mark.gpu
def test_gpu_what_reserve_fmt_refuses(gpu_ctx):
    check_reserve_fmt_refusals(gpu_ctx)


# ---- the host code under ASan + UBSan ----------------------------------------------------------------------------------------------------

@pytest.mark.sanitize
def test_this_file_under_asan_and_ubsan():
    sys.path.insert(0, str(ROOT / "tests" / "emu"))
    import build_emu
    from test_sanitizers import ENV, REPORTS, RUNTIME
    so = build_emu.build_sanitized("asan")
    rt = subprocess.run(["gcc", "-print-file-name=" + RUNTIME["asan"]], capture_output=True, text=True, check=True).stdout.strip()
    preload = " ".join(x for x in (rt, os.environ.get("LD_PRELOAD", "")) if x)  # (in front of whatever is preloaded already, not instead of it)
    env = dict(os.environ, **ENV["asan"], LD_PRELOAD=preload, SYMACCEL_EMU_SANITIZED="asan")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_batcher_output_format.py", "-q", "-x", "-m", "not gpu and not sanitize", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, timeout=2400, env=env, cwd=str(ROOT))
    text = r.stdout + r.stderr
    hits = [ln for ln in text.splitlines() if any(tag in ln for tag in REPORTS)]
    assert so.exists()
    assert not hits, "\n".join(hits[:10]) + text[-3000:]
    assert r.returncode == 0 and " passed" in text, text[-3000:]
