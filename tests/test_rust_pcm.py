"""The Rust side of the PCM output formats, EXECUTED: bindings/rust/symphonia-accel-hip/src/pcm.rs (`SampleFormat`,
`Context::pcm_convert_f32` / `_i32`) under tools/rsinterp with its `extern "C"` calls bound to libsymaccel (the CPU-emulation build here,
the hipcc-built library in the gpu twin), against the numpy restatement of tests/test_pcm_convert.py.

And known answers for the two things the interpreter learned for the fixture of that feature (tools/make_pcm_fixtures.py runs the
reference's `to_ne_sample_bytes`, sample.rs): `cfg!(target_endian = ...)` and the byte images of floats.  As in
tests/test_rsinterp_semantics.py no expectation was read off the interpreter: each is worked from the Rust Reference / std documentation
and IEEE-754 (the working is in the row)."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

from rs_harness import Harness, f32_vec, i32_vec, u8_vec, usize  # noqa: E402
from rsinterp import Interp  # noqa: E402
from rsinterp import interp as I  # noqa: E402
from test_pcm_convert import BYTES, expected  # noqa: E402
from test_rust_adapters import LIBS  # noqa: E402

RUST_NAME = {"u8": "U8", "s8": "S8", "u16": "U16", "s16": "S16", "u24": "U24", "s24": "S24", "u32": "U32", "s32": "S32", "f32": "F32"}


@pytest.mark.parametrize("make_dll", LIBS)
def test_the_rust_wrapper_converts_and_interleaves(make_dll):
    h = Harness(make_dll())
    h.load_shim("ctx.rs", "pcm.rs")
    r = h.it.call("Context::new", I.Int(0, "i32"))
    assert r.variant == "Ok", r
    ctx = r.f["0"]
    rng = np.random.default_rng(5)
    for src, dst, channels, groups, stride, nf in (("f32", "s16", 2, 3, 40, 37), ("f32", "u24", 3, 1, 21, 21), ("s32", "s24", 2, 2, 33, 32), ("s32", "f32", 1, 2, 9, 9),
                                                   ("f32", "u8", 5, 1, 18, 17)):
        planes = (rng.standard_normal((groups * channels, stride)) * 0.7).astype(np.float32) if src == "f32" else \
            rng.integers(-2 ** 31, 2 ** 31, (groups * channels, stride)).astype(np.int32)
        fmt = h.it.resolve_value(["SampleFormat", RUST_NAME[dst]], I.Env(), None)
        assert int(h.it.call_method("SampleFormat", "bytes", fmt).v) == BYTES[dst]
        out = u8_vec(np.full(groups * nf * channels * BYTES[dst] + 5, 0xEE, np.uint8))
        vec = f32_vec(planes) if src == "f32" else i32_vec(planes)
        r = h.it.call_method("Context", "pcm_convert_f32" if src == "f32" else "pcm_convert_i32", ctx, vec, usize(stride), usize(channels), usize(nf), fmt, out)
        assert r.variant == "Ok", r
        got = np.array([b.v for b in out.a], np.uint8)
        assert np.array_equal(got[:-5], expected(src, dst, planes, channels, nf).ravel()), (src, dst)
        assert np.all(got[-5:] == 0xEE)


CFG = "Rust Reference, Conditional compilation, 'target_endian'; the hosts of this project (x86-64, the CPU side of a gfx950 system) are little-endian"
F_BYTES = "std: f32::to_le_bytes / to_be_bytes / to_ne_bytes -- the bytes of to_bits() in that order"

PROBES = [
    ('cfg!(target_endian = "little")', "bool", True, CFG),
    ('cfg!(target_endian = "big")', "bool", False, CFG),
    ('if cfg!(target_endian = "little") { 1u8 } else { 2u8 }', "u8", 1, CFG),
    # 1.0f32 = 0x3F800000
    ("u32::from_le_bytes(1.0f32.to_le_bytes())", "u32", 0x3F800000, F_BYTES),
    ("1.0f32.to_le_bytes()[3] as u32 * 256 + 1.0f32.to_le_bytes()[2] as u32", "u32", 0x3F80, F_BYTES + ": little-endian ends with 0x80, 0x3F"),
    ("1.0f32.to_be_bytes()[0] as u32 * 256 + 1.0f32.to_be_bytes()[1] as u32", "u32", 0x3F80, F_BYTES + ": big-endian starts with 0x3F, 0x80"),
    ("1.0f32.to_ne_bytes()[3] as u32", "u32", 0x3F, F_BYTES + ": native = little here"),
    # -2.5f64 = sign 1, exponent 1 (0x400), fraction 0.25 -> 0xC004000000000000
    ("u64::from_le_bytes((-2.5f64).to_le_bytes())", "u64", 0xC004000000000000, F_BYTES),
    ("(-2.5f64).to_be_bytes()[0] as u32 * 256 + (-2.5f64).to_be_bytes()[1] as u32", "u32", 0xC004, F_BYTES),
    ("(-2.5f64).to_ne_bytes()[7] as u32", "u32", 0xC0, F_BYTES),
    # a NaN keeps its payload: the bytes are the bits
    ("u32::from_le_bytes(f32::from_bits(0x7fc00001).to_le_bytes())", "u32", 0x7FC00001, F_BYTES),
    # the integer case the 24-bit types are built on (sample.rs: the first three of the inner u32's native bytes)
    ("0x00c0ffeeu32.to_ne_bytes()[0] as u32 + 0x00c0ffeeu32.to_ne_bytes()[2] as u32 * 256", "u32", 0xC0EE, "std: u32::to_ne_bytes, little-endian: EE FF C0 00"),
]


@pytest.mark.parametrize("expr,ty,want,source", PROBES, ids=["%02d: %s" % (i, p[0]) for i, p in enumerate(PROBES)])
def test_interpreter_probe(expr, ty, want, source):
    it = Interp()
    it.load_source("pub fn probe() -> %s {\n%s\n}\n" % (ty, expr), "probe.rs")
    got = it.call("probe")
    got = bool(got) if ty == "bool" else int(got.v)
    print("%s -> %r, rustc: %r  [%s]" % (expr, got, want, source))
    assert got == want and type(got) is type(want)
    assert it.overflows == 0
