#!/usr/bin/env python3
"""tests/golden/adpcm.npz: the reference's ADPCM block decoders (symphonia-codec-adpcm/src/codec_ms.rs, codec_ima_wav.rs, codec_ima_qt.rs:
decode_mono / decode_stereo, with common.rs and common_ima.rs) executed under tools/rsinterp, block by block.

    python tools/make_adpcm_fixtures.py            # (needs the reference tree) writes the fixture
    python tools/make_adpcm_fixtures.py --check    # regenerates and compares

Each codec file runs in an interpreter of its own (the three files define functions of the same names).  The fixture holds data only:
per case the blocks (uint8[n, block bytes]), what the reference decoded them to (int32[n, channels, frames_per_block]) and, in the
manifest, the number of implicit integer wraps the interpreter counted (a debug build of the reference would have panicked there; the
release build wraps, and so does the interpreter).  The cases:

  enc_*    packets of the test-side encoder (tests/adpcm_writer.py) for a synthetic signal: overflows == 0, asserted;
  edge_*   hand-made blocks: every nibble value, step index at 0 and 88 and clamped at both, predictors at the i16 limits and clamps hit
           on both sides, all seven MS predictors, a negative initial MS delta, the QT header masks: overflows == 0, asserted;
  rand_*   arbitrary bytes for the IMA codecs (they cannot overflow: asserted);
  wrap_ms_* arbitrary bytes for MS: delta grows until T[n] * delta and signed_nibble * delta leave 32 bits; recorded WITH the count.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

OUT = ROOT / "tests" / "golden" / "adpcm.npz"
CRATE = "symphonia-codec-adpcm/src/"
FILES = {"ms": "codec_ms.rs", "ima_wav": "codec_ima_wav.rs", "ima_qt": "codec_ima_qt.rs"}
DRIVER = """
pub fn adpcm_fixture_mono(data: &[u8], fpb: usize) -> Vec<i32> {
    let mut r = BufReader::new(data); let mut buf = vec![0i32; fpb]; decode_mono(&mut r, &mut buf, fpb).unwrap(); buf }
pub fn adpcm_fixture_stereo(data: &[u8], fpb: usize) -> Vec<i32> {
    let mut r = BufReader::new(data); let mut l = vec![0i32; fpb]; let mut rr = vec![0i32; fpb];
    decode_stereo(&mut r, [&mut l, &mut rr], fpb).unwrap(); l.extend_from_slice(&rr); l }
"""


def le16(v):
    return [v & 0xff, (v >> 8) & 0xff]


def nibble_bytes(nibbles, upper_first):
    """pairs of nibbles -> bytes"""
    n = list(nibbles)
    return [(a << 4 | b) if upper_first else (b << 4 | a) for a, b in zip(n[0::2], n[1::2])]


def edge_ima_wav():
    """mono, 33 frames (16 data bytes, 32 nibbles)"""
    every = list(range(16)) + list(range(15, -1, -1))
    rows = [
        le16(32767) + [88, 0] + nibble_bytes([7] * 32, False),                 # the top clamp, the index held at 88
        le16(-32768 & 0xffff) + [88, 0] + nibble_bytes([15] * 32, False),      # the bottom clamp
        le16(0) + [0, 0] + nibble_bytes([8, 0] * 16, False),                   # the index held at 0
        le16(1234) + [40, 0] + nibble_bytes(every, False),                     # every nibble value
        le16(-32768 & 0xffff) + [0, 255] + nibble_bytes([7, 7, 7, 7, 15, 15, 15, 15] * 4, False),  # up from the floor and back, a set reserved byte
        le16(32767) + [87, 0] + nibble_bytes([4, 12] * 16, False),             # 87 + 2 clamps to 88
    ]
    return np.array(rows, np.uint8), 1, 33


def edge_ima_wav_stereo():
    """stereo, 17 frames: the two channels at opposite limits"""
    rows = [le16(32767) + [88, 0] + le16(-32768 & 0xffff) + [88, 7] + [0x77] * 4 + [0xff] * 4 + [0xff] * 4 + [0x77] * 4,
            le16(0) + [0, 0] + le16(0xffff) + [1, 0] + [0x80, 0x08, 0x10, 0x32] + [0x54, 0x76, 0x98, 0xba] + [0xdc, 0xfe, 0x00, 0x88] + [0x0f, 0xf0, 0x3c, 0xc3]]
    return np.array(rows, np.uint8), 2, 17


def edge_ima_qt():
    every = nibble_bytes(list(range(16)) * 4, False)
    rows = [[0xff, 0xff] + [0x77] * 32,        # predictor 0xff80 = -128, index 127 -> 88
            [0x7f, 0xff] + [0x77] * 32,        # predictor 0x7f80, the top clamp
            [0x80, 0x00] + [0xff] * 32,        # predictor -32768, index 0, the bottom clamp
            [0x00, 0x58] + every,              # index exactly 88
            [0x12, 0x34 | 0x80] + every,       # the low predictor bit set in the header: masked off
            [0x00, 0x00] + [0x08, 0x80] * 16]  # index held at 0
    return np.array(rows, np.uint8), 1, 64


def edge_ms():
    """mono, 34 frames (16 data bytes)"""
    rows = []
    for pi in range(7):  # every predictor, every nibble value
        rows.append([pi] + le16(16) + le16(1000 - 300 * pi & 0xffff) + le16(-700 + 250 * pi & 0xffff) + nibble_bytes(list(range(16)) + list(range(15, -1, -1)), True))
    rows.append([0] + le16(20000) + le16(30000) + le16(30000) + nibble_bytes([3, 3, 13, 13, 13, 13, 3, 3] * 4, True))            # both clamps
    rows.append([1] + le16(-100 & 0xffff) + le16(5) + le16(-5 & 0xffff) + nibble_bytes([1, 15, 2, 14, 7, 8, 0, 4] * 4, True))     # a negative initial delta
    rows.append([1] + le16(16) + le16(32767) + le16(-32768 & 0xffff) + nibble_bytes([0] * 32, True))                             # 2 * s1 - s2 beyond i16 in both directions
    rows.append([5] + le16(-32768 & 0xffff) + le16(-32768 & 0xffff) + le16(32767) + nibble_bytes([1, 15] * 16, True))            # the most negative delta
    return np.array(rows, np.uint8), 1, 34


def edge_ms_stereo():
    rows = [[6, 1] + le16(17) + le16(-3 & 0xffff) + le16(32767) + le16(-32768 & 0xffff) + le16(-32768 & 0xffff) + le16(32767) + [0x3d, 0xd3, 0x71, 0x17, 0x88, 0x00, 0xf0, 0x0f, 0x2e, 0xe2],
            [0, 4] + le16(2000) + le16(2000) + le16(100) + le16(-100 & 0xffff) + le16(0) + le16(50) + [0x11, 0xff, 0x35, 0x53, 0xdd, 0xdd, 0x33, 0x33, 0x0f, 0xf0]]
    return np.array(rows, np.uint8), 2, 12


def cases():
    """(name, codec, blocks, channels, frames per block, may the reference wrap)"""
    import adpcm_writer as W
    from adpcm_ref import block_bytes, CODECS
    out = []
    for codec, ch, fpb, n in (("ms", 1, 132, 8), ("ms", 2, 75, 8), ("ima_wav", 1, 131, 6), ("ima_wav", 2, 73, 6), ("ima_qt", 1, 64, 7), ("ima_qt", 2, 64, 5)):
        pcm = W.signal(11 * ch + len(codec), ch, n * fpb)
        blocks = W.encode_ms(pcm, fpb) if codec == "ms" else (W.encode_ima_wav(pcm, fpb) if codec == "ima_wav" else W.encode_ima_qt(pcm))
        out.append(("enc_%s_%d" % (codec, ch), codec, blocks, ch, fpb, False))
    for name, codec, (blocks, ch, fpb) in (("edge_ima_wav_1", "ima_wav", edge_ima_wav()), ("edge_ima_wav_2", "ima_wav", edge_ima_wav_stereo()),
                                            ("edge_ima_qt_1", "ima_qt", edge_ima_qt()), ("edge_ms_1", "ms", edge_ms()), ("edge_ms_2", "ms", edge_ms_stereo())):
        out.append((name, codec, blocks, ch, fpb, False))
    rng = np.random.default_rng(2026)
    for codec, ch, fpb, n in (("ima_wav", 1, 67, 5), ("ima_wav", 2, 25, 5), ("ima_qt", 2, 64, 4)):
        blocks = rng.integers(0, 256, (n, block_bytes(CODECS[codec], ch, fpb)), dtype=np.uint8)
        if codec == "ima_wav":
            blocks[:, 2] %= 89
            blocks[:, 6] %= 89 if ch == 2 else 255
        out.append(("rand_%s_%d" % (codec, ch), codec, blocks, ch, fpb, False))
    for ch, fpb, n in ((1, 66, 5), (2, 41, 5)):
        blocks = rng.integers(0, 256, (n, block_bytes(CODECS["ms"], ch, fpb)), dtype=np.uint8)
        blocks[:, :ch] %= 7
        out.append(("wrap_ms_%d" % ch, "ms", blocks, ch, fpb, True))
    return out


def interpreter(codec):
    import rs_harness as H
    from rsinterp import Interp
    it = Interp()
    for f in H.CORE_IO:
        it.load_source((H.REF / "symphonia-core/src" / f).read_text(), "symphonia-core/src/" + f)
    for f in ("common.rs", "common_ima.rs", FILES[codec]):
        it.load_source((H.REF / CRATE / f).read_text(), CRATE + f)
    assert not it.globals.get("__unparsed__"), it.globals.get("__unparsed__")
    it.load_source(DRIVER, "adpcm_fixture_driver.rs")
    return it


def generate():
    """{name: array} as the fixture file holds them (needs the reference tree)"""
    import rs_harness as H
    its = {c: interpreter(c) for c in FILES}
    out, entries = {}, []
    for name, codec, blocks, ch, fpb, may_wrap in cases():
        it = its[codec]
        before = it.overflows
        pcm = np.zeros((len(blocks), ch, fpb), np.int32)
        for i, b in enumerate(blocks):
            r = it.call("adpcm_fixture_mono" if ch == 1 else "adpcm_fixture_stereo", H.u8_vec(b), H.usize(fpb))
            pcm[i] = np.array([x.v for x in r.a], np.int64).astype(np.int32).reshape(ch, fpb)
        wraps = it.overflows - before
        assert may_wrap or wraps == 0, "%s: %d implicit integer wraps: a debug build of the reference would have panicked" % (name, wraps)
        assert not may_wrap or wraps > 0, "%s: arbitrary MS bytes were meant to overflow" % name
        out[name + "_bytes"], out[name + "_pcm"] = blocks, pcm
        entries.append({"name": name, "codec": codec, "channels": ch, "frames_per_block": fpb, "blocks": int(len(blocks)), "overflows": int(wraps),
                        "ref": CRATE + FILES[codec] + (":decode_mono" if ch == 1 else ":decode_stereo")})
    manifest = {"generator": "tools/make_adpcm_fixtures.py", "entries": entries, "also": [CRATE + "common.rs", CRATE + "common_ima.rs:38-48 (expand_nibble)"]}
    out["manifest"] = np.frombuffer(json.dumps(manifest, indent=1, sort_keys=True).encode(), np.uint8).copy()
    return out


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
    m = json.loads(bytes(got["manifest"]).decode())
    for e in m["entries"]:
        print("%-16s %-8s ch %d fpb %4d blocks %2d overflows %d" % (e["name"], e["codec"], e["channels"], e["frames_per_block"], e["blocks"], e["overflows"]))
    print("%s: %d bytes" % (OUT, OUT.stat().st_size))


if __name__ == "__main__":
    main()
