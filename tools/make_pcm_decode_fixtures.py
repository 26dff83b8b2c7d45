#!/usr/bin/env python3
"""tests/golden/pcm_decode.npz: the sample arithmetic of symphonia-codec-pcm, executed from the reference tree under tools/rsinterp.

    python tools/make_pcm_decode_fixtures.py            # (needs the reference tree) writes the fixture
    python tools/make_pcm_decode_fixtures.py --check    # regenerates and compares

Two parts.

PACKETS (`dec_*`): the reference's own decoder.  `PcmDecoder::try_new` and `decode_ref` of symphonia-codec-pcm/src/lib.rs run whole, on
symphonia-core's own io/, packet.rs, audio/sample.rs and audio/conv.rs, for all twenty codecs, one to eight channels, shift 0 and (integer
codecs) a shift set through bits_per_sample / bits_per_coded_sample.  One decoder per case takes a sequence of packets: a long one, a
short one after it, an empty one, one frame, a trailing partial frame, and one longer than max_frames_per_packet -- every packet but the
last lies below max_frames_per_packet, which is the swallowed-underrun path of lib.rs:328 over audio/buf.rs:318-346.  Recorded per packet:
the bytes, the frame count the buffer holds, the buffer's variant and its planes (floats as their bits).  Also recorded: the Error variant
and message of every refusal of try_new (lib.rs:220-303).  Stand-ins, not reference text: AudioBuffer / GenericAudioBuffer / AudioSpec
(tests/rust/audio_stubs.rs, tests/rust/pcm_stubs.rs: same signatures, render_with and grow_capacity with the reference's logic), and ONE
edit of lib.rs in memory: `($read << $shift).into_sample()` (lib.rs:58, 76) becomes `pcm_stub_into_sample(SampleFormat::$fmt, $read <<
$shift)`, which calls `<sample type of $fmt>::from_sample` -- what IntoSample forwards to (conv.rs:632-637) -- because the interpreter does
not track the type an expression is assigned to.  The interpreter gained f32 / f64 `from_{le,be}_bytes` for the float reads.

SAMPLES AND CONVERSIONS: the reads of symphonia-core/src/io, `<<`, FromSample and alaw_to_linear / mulaw_to_linear driven sample by sample
by the driver below (all 256 codes of the 1-byte codecs, several shifts), and FromSample of conv.rs:461-621 for the eight sample types
PcmDecoder adds as sources.

The fixture holds data only; the manifest records the interpreter's count of implicit integer wraps (0, asserted).
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

OUT = ROOT / "tests" / "golden" / "pcm_decode.npz"
CONV = "symphonia-core/src/audio/conv.rs"
LIB = "symphonia-codec-pcm/src/lib.rs"
# codec -> (the read of lib.rs:328-388, the buffer's sample type, how the native sample leaves as an integer)
READS = {
    "s32le": ("r.read_i32()", "i32", "s"), "s32be": ("r.read_be_i32()", "i32", "s"),
    "s24le": ("r.read_i24()", "i24", "s.inner()"), "s24be": ("r.read_be_i24()", "i24", "s.inner()"),
    "s16le": ("r.read_i16()", "i16", "s"), "s16be": ("r.read_be_i16()", "i16", "s"), "s8": ("r.read_i8()", "i8", "s"),
    "u32le": ("r.read_u32()", "u32", "s"), "u32be": ("r.read_be_u32()", "u32", "s"),
    "u24le": ("r.read_u24()", "u24", "s.inner()"), "u24be": ("r.read_be_u24()", "u24", "s.inner()"),
    "u16le": ("r.read_u16()", "u16", "s"), "u16be": ("r.read_be_u16()", "u16", "s"), "u8": ("r.read_u8()", "u8", "s"),
}
RUST = {"u8": "u8", "s8": "i8", "u16": "u16", "s16": "i16", "u24": "u24", "s24": "i24", "u32": "u32", "s32": "i32", "f32": "f32", "f64": "f64"}
NEW_SOURCES = ("s8", "s16", "s24", "u8", "u16", "u24", "u32", "f64")


def driver():
    fns = []
    for codec, (read, ty, leave) in READS.items():
        value = "(v << 8)" if "24" in codec else "v"  # lib.rs:336-360: the 24-bit reads are shifted up by 8 first
        fns.append("pub fn pcmfix_%s(data: &[u8], shift: u32) -> Vec<i64> { let mut r = BufReader::new(data); let mut o = Vec::new(); loop { "
                   "let v = match %s { Ok(v) => v, Err(_) => break }; let s: %s = %s::from_sample(%s << shift); o.push(%s as i64); } o }"
                   % (codec, read, ty, ty, value, leave))
    for law in ("alaw", "mulaw"):
        fns.append("pub fn pcmfix_%s(data: &[u8], shift: u32) -> Vec<i64> { let mut o = Vec::new(); for &b in data.iter() { let s: i16 = %s_to_linear(b); "
                   "o.push(s as i64); } o }" % (law, law))
    make = {"s8": "x as i8", "s16": "x as i16", "s24": "i24::from(x as i32)", "u8": "x as u8", "u16": "x as u16", "u24": "u24::from(x as u32)",
            "u32": "x as u32", "f64": "f64::from_bits(x as u64)"}
    import pcm_decode_ref as R
    for src in NEW_SOURCES:
        for dst in R.DESTS:
            fns.append("pub fn pcmfix_%s_to_%s(v: &[i64]) -> Vec<u8> { let mut o = Vec::new(); for &x in v.iter() { let s: %s = %s; let b = %s::from_sample(s)"
                       ".to_ne_sample_bytes(); for y in b.iter() { o.push(*y); } } o }" % (src, dst, RUST[src], make[src], RUST[dst]))
    return "\n".join(fns) + "\n"


def log_functions():
    """lib.rs:150-181: the constants and the two expansions, cut from the reference file where it stands"""
    text = (__import__("rs_harness").REF / LIB).read_text()
    a, b = text.index("const XLAW_QUANT_MASK"), text.index("fn is_supported_pcm_codec")
    return text[a:b]


def sample_inputs(fam, rng):
    """native samples of a family as int64 (f64: the bits): the ends, the middle, steps across the destination's rounding, arbitrary ones"""
    import pcm_decode_ref as R
    if fam == "f64":
        vals = [0.0, -0.0, 1.0, -1.0, 1.0 + 2 ** -52, -1.0 - 2 ** -52, 2.0, -2.0, 1e300, -1e300, float("inf"), float("-inf"), 5e-324, -5e-324, 2 ** -1022,
                0.5, -0.5, 1.0 - 2 ** -53, -1.0 + 2 ** -53, 1 / 3, -1 / 3, 127 / 128, 32767 / 32768, 8388607 / 8388608, 2147483647 / 2147483648,
                (2 ** 31 - 0.5) / 2 ** 31, 1e-10, -1e-10, 3.0000001e-5,
                1e-40, -1e-40, 2 ** -126, 2 ** -127, 2 ** -149, 2 ** -150, 1.5 * 2 ** -149, 3.4028234663852886e38, 3.4028235677973366e38, -3.5e38]
        x = np.concatenate([np.array(vals, np.float64), rng.standard_normal(160) * 0.7, rng.uniform(-1, 1, 160), (rng.integers(-2 ** 23, 2 ** 23, 80) + 0.5) / 2 ** 23])
        bits = x.view(np.uint64).astype(np.int64) if False else x.view(np.int64).copy()
        nan = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0x7ff4000020000001, 0xfff7ffffffffffff], np.uint64).view(np.int64)
        return np.concatenate([bits, nan])
    w, signed = R.WIDTH[fam], fam[0] == "s"
    lo, hi = (-(1 << (w - 1)), (1 << (w - 1)) - 1) if signed else (0, (1 << w) - 1)
    if w == 8:
        return np.arange(lo, hi + 1, dtype=np.int64)
    edge = np.array([lo, lo + 1, lo + 255, lo + 256, -1 if signed else (1 << (w - 1)) - 1, 0 if signed else 1 << (w - 1), 1 if signed else (1 << (w - 1)) + 1, hi - 256, hi - 255, hi - 1, hi], np.int64)
    return np.concatenate([edge, rng.integers(lo, hi + 1, 400, dtype=np.int64)])


def generate():
    """{name: array} as the fixture file holds them (needs the reference tree)"""
    import pcm_decode_ref as R
    import rs_harness as H
    it = H.reference_test_interp(CONV)
    for f in H.CORE_IO:
        if f != "util.rs":
            it.load_source((H.REF / "symphonia-core/src" / f).read_text(), "symphonia-core/src/" + f)
    it.load_source(log_functions(), LIB + ":150-181")
    assert not it.globals.get("__unparsed__"), it.globals.get("__unparsed__")
    it.load_source(driver(), "pcm_decode_fixture_driver.rs")
    rng = np.random.default_rng(2026)
    out, entries = {}, []
    for codec in list(READS) + ["alaw", "mulaw"]:
        cb, kind, _, fam = R.CODECS[codec]
        w = R.WIDTH[fam]
        shifts = (0,) if kind not in "su" else tuple(sorted({0, 1, w // 2 - 1, w - 8, w - 1} - {-1} if w > 8 else {0, 1, 3, 7}))
        for shift in shifts:
            if cb == 1:
                data = np.arange(256, dtype=np.uint8)
            else:
                ends = np.array([[0] * cb, [0xff] * cb, [0x80] + [0] * (cb - 1), [0] * (cb - 1) + [0x80], [0x7f] + [0xff] * (cb - 1), [0xff] * (cb - 1) + [0x7f],
                                 list(range(1, cb + 1))], np.uint8)
                data = np.concatenate([ends.ravel(), rng.integers(0, 256, 57 * cb, dtype=np.uint8), np.array([0x12], np.uint8)])  # (a trailing partial sample: the read fails)
            r = it.call("pcmfix_" + codec, H.u8_vec(data), I_u32(shift))
            name = "%s_sh%d" % (codec, shift)
            out[name + "_bytes"] = data
            out[name + "_native"] = np.array([x.v for x in r.a], np.int64).astype(R.NATIVE_DTYPE[fam])
            assert len(r.a) == len(data) // cb
            entries.append({"name": name, "codec": codec, "shift": shift, "samples": len(r.a), "ref": LIB})
    for src in NEW_SOURCES:
        x = sample_inputs(src, rng)
        out["in_" + src] = x
        for dst in R.DESTS:
            r = it.call("pcmfix_%s_to_%s" % (src, dst), I_i64_vec(x))
            out["%s_to_%s" % (src, dst)] = np.array([b.v for b in r.a], np.uint8).reshape(len(x), R.DEST_BYTES[dst])
            entries.append({"name": "%s_to_%s" % (src, dst), "cases": int(len(x)), "ref": CONV})
    refusals, wraps = generate_packets(out, entries)
    assert it.overflows == 0 and wraps == 0, "%d implicit integer wraps: a debug build of the reference would have panicked" % (it.overflows + wraps)
    manifest = {"generator": "tools/make_pcm_decode_fixtures.py", "entries": entries, "overflows": int(it.overflows + wraps), "try_new_refusals": refusals,
                "also": ["symphonia-core/src/io/mod.rs:152-260", "symphonia-core/src/io/buf_reader.rs", "symphonia-core/src/audio/sample.rs", "symphonia-core/src/util.rs:222-275"]}
    out["manifest"] = np.frombuffer(json.dumps(manifest, indent=1, sort_keys=True).encode(), np.uint8).copy()
    return out


FLOAT_SPECIALS = {4: [0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0xffa55aa5, 0x3f800000, 0xbf7fffff, 0x00800000],
                  8: [0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x800fffffffffffff, 0x7ff0000000000000, 0xfff0000000000000,
                      0x7ff8000000000000, 0x7ff0000000000001, 0xfff5a5a5a5a5a5a5, 0x3ff0000000000000, 0xbfefffffffffffff, 0x36a0000000000000,
                      0x380fffffffffffff, 0x47efffffffffffff, 0x47f0000000000000]}
MAX_FRAMES = 12
TRY_NEW_REFUSALS = (  # codec, rate, channels, bits_per_sample, bits_per_coded_sample
    ("CODEC_ID_FLAC", 8000, 1, None, None), ("CODEC_ID_PCM_S16LE", None, 1, None, None), ("CODEC_ID_PCM_S16LE", 8000, None, None, None),
    ("CODEC_ID_PCM_S16LE", 8000, 1, None, 17), ("CODEC_ID_PCM_S16LE", 8000, 1, 17, None), ("CODEC_ID_PCM_S16LE", 8000, 1, 12, 13),
    ("CODEC_ID_PCM_S24BE", 8000, 2, 25, None), ("CODEC_ID_PCM_F32LE", 8000, 1, 24, None), ("CODEC_ID_PCM_F32LE", 8000, 1, None, 24),
    ("CODEC_ID_PCM_F64BE", 8000, 1, 32, 32), ("CODEC_ID_PCM_ALAW", 8000, 1, 8, None), ("CODEC_ID_PCM_MULAW", 8000, 1, 16, 8), ("CODEC_ID_PCM_U8", 8000, 1, None, 9))


def decoder_harness():
    import rs_harness as H
    h = H.Harness(None, reference=True, sample="i32")
    h.it.load_file(ROOT / "tests" / "rust" / "pcm_stubs.rs")
    for f in ("audio/sample.rs", "audio/conv.rs"):
        h.it.load_file(H.REF / "symphonia-core" / "src" / f)
    text = (H.REF / LIB).read_text()
    old = "plane[idx] = ($read << $shift).into_sample();"
    assert text.count(old) == 2  # read_pcm_signed, read_pcm_unsigned
    h.it.load_source(text.replace(old, "plane[idx] = pcm_stub_into_sample(SampleFormat::$fmt, $read << $shift);"), LIB)
    assert not h.it.globals.get("__unparsed__"), h.it.globals.get("__unparsed__")
    return h


def pcm_params(h, codec_id, rate, nch, bps, bpcs, max_frames):
    from rsinterp import interp as I
    p = h.params(codec_id, rate=rate, nch=nch, bps=bps)
    p.f["bits_per_coded_sample"] = I.some(I.Int(bpcs, "u32")) if bpcs else I.NONE
    p.f["max_frames_per_packet"] = I.some(I.Int(max_frames, "u64")) if max_frames else I.NONE
    return p


def sample_bits(v, dtype):
    """one sample of a plane as the interpreter holds it -> an integer"""
    import struct
    from rsinterp import interp as I
    v = I.deref(v)
    if isinstance(v, np.float32):
        return int(v.view(np.uint32))
    if isinstance(v, float):
        return struct.unpack("<Q", struct.pack("<d", v))[0]
    if isinstance(v, I.Struct):  # i24 / u24
        return int(I.deref(v.f["0"]).v)
    return int(v.v)


def generate_packets(out, entries):
    """the reference's PcmDecoder on packet sequences -> arrays into `out`, manifest entries into `entries`; returns the refusals of try_new"""
    import pcm_decode_ref as R
    from rsinterp import interp as I
    h = decoder_harness()
    it = h.it
    rng = np.random.default_rng(1320)
    for k, codec in enumerate(R.NAMES):
        cb, kind, _, fam = R.CODECS[codec]
        w = R.WIDTH[fam]
        ch = (1, 2, 3, 8)[k % 4] if codec not in ("s24le", "s24be") else 3  # (3-byte samples in 3 channels: a 9-byte frame)
        for shift in ((0, (w // 2 + 3) % w) if kind in "su" else (0,)):
            bps, bpcs = (w, w - shift) if shift else (None, None)
            r = it.call("PcmDecoder::try_new", pcm_params(h, "CODEC_ID_PCM_" + codec.upper(), 8000, ch, bps, bpcs, MAX_FRAMES), h.opts())
            assert r.variant == "Ok", (codec, r)
            dec = r.f["0"]
            assert int(I.deref(I.deref(dec).f["shift"]).v) == shift
            fb = cb * ch
            lens = [9 * fb, 4 * fb, 0, fb, 5 * fb + fb - 1, fb - 1 if fb > 1 else 0, (MAX_FRAMES + 3) * fb, 2 * fb]
            name = "dec_%s_sh%d" % (codec, shift)
            packets = []
            for j, n in enumerate(lens):
                data = rng.integers(0, 256, n, dtype=np.uint8)
                if kind == "f" and j == 6:  # the specials, in the codec's byte order
                    sp = np.array(FLOAT_SPECIALS[cb], "<u4" if cb == 4 else "<u8").view(np.uint8).reshape(-1, cb)
                    sp = (sp[:, ::-1] if codec.endswith("be") else sp).ravel()
                    data[:len(sp)] = sp[:n]
                rr = it.call_method("PcmDecoder", "decode_ref", dec, h.packet(data, j))
                assert rr.variant == "Ok", (codec, j, rr)
                g = I.deref(rr.f["0"])
                buf = I.deref(g.f["0"])
                frames = int(I.deref(buf.f["num_frames"]).v)
                planes = [I.deref(pl).a[:frames] for pl in I.deref(buf.f["planes"]).a]
                assert len(planes) == ch
                bits = np.array([[sample_bits(v, fam) for v in pl] for pl in planes], np.int64 if fam != "f64" else np.uint64).reshape(ch, frames)
                store = {"f32": np.uint32, "f64": np.uint64}.get(fam, R.NATIVE_DTYPE[fam])
                out["%s_p%d_bytes" % (name, j)] = data
                out["%s_p%d_planes" % (name, j)] = bits.astype(store)
                packets.append({"len": int(n), "frames": frames, "variant": g.variant})
            entries.append({"name": name, "decoder": "PcmDecoder::try_new + decode_ref", "codec": codec, "channels": ch, "shift": shift,
                            "max_frames_per_packet": MAX_FRAMES, "packets": packets, "ref": LIB})
    refusals = []
    for codec_id, rate, nch, bps, bpcs in TRY_NEW_REFUSALS:
        r = it.call("PcmDecoder::try_new", pcm_params(h, codec_id, rate, nch, bps, bpcs, None), h.opts())
        assert r.variant == "Err", (codec_id, rate, nch, bps, bpcs)
        e = I.deref(r.f["0"])
        msg = I.deref(e.f["0"])
        refusals.append({"codec": codec_id, "sample_rate": rate, "channels": nch, "bits_per_sample": bps, "bits_per_coded_sample": bpcs,
                         "error": e.variant, "message": msg if isinstance(msg, str) else str(getattr(msg, "s", msg))})
    return refusals, it.overflows


def I_u32(v):
    from rsinterp import interp as I
    return I.Int(int(v), "u32")


def I_i64_vec(a):
    from rsinterp import interp as I
    return I.Arr([I.Int(int(x), "i64") for x in np.asarray(a).ravel()], True)


def compare(want, have):
    """names whose arrays differ between two fixture dicts"""
    return sorted(k for k in set(want) | set(have) if k not in want or k not in have or want[k].shape != have[k].shape or not np.array_equal(want[k], have[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    got = generate()
    if a.check:
        bad = compare(got, dict(np.load(OUT)))
        print("differs: %s" % bad if bad else "%s matches the reference" % OUT.name)
        raise SystemExit(1 if bad else 0)
    np.savez_compressed(OUT, **got)
    print("%s: %d arrays, %d bytes" % (OUT, len(got), OUT.stat().st_size))


if __name__ == "__main__":
    main()
