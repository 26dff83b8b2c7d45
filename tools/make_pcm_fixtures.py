"""tests/golden/pcm_convert.npz: the reference's sample-format conversions (symphonia-core/src/audio/conv.rs, FromSample) executed under
tools/rsinterp, for the 18 (source, destination) pairs symaccel_pcm_convert offers.

    python tools/make_pcm_fixtures.py            # needs the reference tree; writes the fixture
    python tools/make_pcm_fixtures.py --check    # regenerates in memory and compares with the committed file

The file holds data only: the inputs (`in_f32` as bit patterns, `in_i32`), for every pair the bytes `to_ne_sample_bytes()` gives for the
converted sample on a little-endian host (`f32_to_s16`: uint8[n, 2], ...), and `manifest` (JSON: the file:line of every reference item
executed).  The driver below is this project's text; the conversions, the clamp and the 24-bit types are the reference's, loaded from
its tree with the siblings tests/rs_harness.py lists for audio/conv.rs.

The 16-bit sweep of tests/test_pcm_convert.py (every k / 32768 and its two neighbours, about 4 x 10^5 floats) would be tens of megabytes
here; the fixture carries every 61st step of it (all steps near both ends and near zero), a few hundred 24-bit steps, the special values
and the i32 cases in full.  The test checks its numpy restatement against the fixture, and the kernel against both.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

OUT = ROOT / "tests" / "golden" / "pcm_convert.npz"
CONV = "symphonia-core/src/audio/conv.rs"
DESTS = ("u8", "s8", "u16", "s16", "u24", "s24", "u32", "s32", "f32")  # the order of SYMACCEL_FMT_*
RUST = {"u8": "u8", "s8": "i8", "u16": "u16", "s16": "i16", "u24": "u24", "s24": "i24", "u32": "u32", "s32": "i32", "f32": "f32"}
BYTES = {"u8": 1, "s8": 1, "u16": 2, "s16": 2, "u24": 3, "s24": 3, "u32": 4, "s32": 4, "f32": 4}
LINES = {  # what each pair executes
    "f32": {"u8": 596, "u16": 597, "u24": 598, "u32": 599, "s8": 601, "s16": 602, "s24": 603, "s32": 604, "f32": 606},
    "s32": {"u8": 521, "u16": 522, "u24": 523, "u32": 524, "s8": 526, "s16": 527, "s24": 528, "s32": 529, "f32": 531},
}


def neighbours(x):
    """x and the floats next to it, as float32"""
    x = np.asarray(x, np.float32)
    return np.stack([np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))], axis=-1).ravel()


def special_f32():
    bits = [0x00000000, 0x80000000, 0x3f800000, 0xbf800000, 0x3f7fffff, 0x3f800001, 0xbf7fffff, 0xbf800001,  # +-0, +-1 and the floats beside them
            0x7fc00000, 0xffc00000, 0x7f800001, 0xffbfffff,  # NaN of both signs, quiet and signalling
            0x7f800000, 0xff800000,  # +-inf
            0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000,  # the denormals' ends, the smallest normals
            0x7f7fffff, 0xff7fffff,  # +-FLT_MAX
            0x3f000000, 0xbf000000, 0x40000000, 0xc0000000, 0x3eaaaaab, 0xbeaaaaab]
    return np.array(bits, np.uint32).view(np.float32)


def steps16(stride=1):
    """k / 32768 for k in -32770 .. 32770 (every `stride`-th, and every one within 40 of -32768, 0 and 32768) with both neighbours"""
    k = np.arange(-32770, 32771)
    if stride > 1:
        keep = (k % stride == 0) | (np.abs(k) < 40) | (np.abs(np.abs(k) - 32768) < 40)
        k = k[keep]
    return neighbours(k.astype(np.float32) / np.float32(32768.0))


def steps24(count=300, seed=24):
    rng = np.random.default_rng(seed)
    k = np.concatenate([rng.integers(-8388608, 8388609, count), [-8388609, -8388608, -8388607, -1, 0, 1, 8388606, 8388607, 8388608, 8388609]])
    return neighbours(k.astype(np.float64) / 8388608.0)


def inputs_i32():
    v = [0, 1, -1, 2**31 - 1, -2**31, -2**31 + 1, 0x01234567, -0x01234567, 0x7f, 0x80, 0xff, 0x100, 0x7fff, 0x8000, 0x7fffff, 0x800000]
    for p in range(31):
        v += [2**p - 1, 2**p, 2**p + 1, -(2**p) - 1, -(2**p), -(2**p) + 1]
    v += [int(x) for x in np.random.default_rng(32).integers(-2**31, 2**31, 64)]
    return np.array([x for x in v if -2**31 <= x < 2**31], np.int64).astype(np.int32)


def inputs_f32():
    rng = np.random.default_rng(7)
    return np.concatenate([special_f32(), steps16(61), steps24(), (rng.standard_normal(256) * 0.7).astype(np.float32)]).astype(np.float32)


def driver():
    fns = []
    for src in ("f32", "s32"):
        for dst in DESTS:
            fns.append("pub fn pcm_fixture_%s_to_%s(v: &[%s]) -> Vec<u8> { let mut o = Vec::new(); for &s in v.iter() { let b = %s::from_sample(s)"
                       ".to_ne_sample_bytes(); for x in b.iter() { o.push(*x); } } o }" % (src, dst, RUST[src], RUST[dst]))
    return "\n".join(fns) + "\n"


def generate():
    """{name: array} as the fixture file holds them (needs the reference tree)"""
    import rs_harness as H
    it = H.reference_test_interp(CONV)
    it.load_source(driver(), "pcm_fixture_driver.rs")
    xf, xi = inputs_f32(), inputs_i32()
    out = {"in_f32": xf.view(np.uint32).copy(), "in_i32": xi}
    entries = []
    for src, x, vec in (("f32", xf, H.f32_vec), ("s32", xi, H.i32_vec)):
        for dst in DESTS:
            r = it.call("pcm_fixture_%s_to_%s" % (src, dst), vec(x))
            out["%s_to_%s" % (src, dst)] = np.array([b.v for b in r.a], np.uint8).reshape(len(x), BYTES[dst])
            entries.append({"pair": "%s_to_%s" % (src, dst), "cases": int(len(x)), "ref": "%s:%d" % (CONV, LINES[src][dst])})
    assert it.overflows == 0, "%d implicit integer wraps: a debug build of the reference would have panicked" % it.overflows
    manifest = {"generator": "tools/make_pcm_fixtures.py", "entries": entries,
                "also": ["symphonia-core/src/util.rs:258-266 (clamp_f32)", "symphonia-core/src/util.rs:222-237 (clamp_u24, clamp_i24)",
                         "symphonia-core/src/audio/sample.rs:272-276, 457-461 (i24 / u24 from i32 / u32)",
                         "symphonia-core/src/audio/sample.rs:252-262, 437-447 (to_ne_bytes of i24 / u24, little-endian)",
                         "%s:516-519 (i32_to_u32)" % CONV]}
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
    print("%s: %d f32 and %d i32 inputs, %d bytes" % (OUT, len(got["in_f32"]), len(got["in_i32"]), OUT.stat().st_size))


if __name__ == "__main__":
    main()
