"""The Rust side of the PCM / G.711 decode, EXECUTED: bindings/rust/symphonia-accel-hip/src/pcmdec.rs (`PcmCodec`, the map from the
reference's codec ids, `Context::pcm_decode`, `Context::pcm_decode_as`) under tools/rsinterp with its `extern "C"` calls bound to
libsymaccel (the CPU-emulation build here, the hipcc-built library in the gpu twin), against the numpy restatement of
tests/pcm_decode_ref.py (pinned to the reference fixture by tests/test_pcm_decode.py); and the shim's import / declaration checks:
symaccel_sys.rs declares what the module calls, lib.rs names the module, `register()` still lists its five codecs."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import pcm_decode_ref as R  # noqa: E402
from rs_harness import Harness, u8_vec, usize  # noqa: E402
from rsinterp import interp as I  # noqa: E402
from test_rust_adapters import LIBS  # noqa: E402

CRATE = ROOT / "bindings" / "rust" / "symphonia-accel-hip" / "src"
RUST_NAME = {"s32le": "S32Le", "s32be": "S32Be", "s24le": "S24Le", "s24be": "S24Be", "s16le": "S16Le", "s16be": "S16Be", "s8": "S8", "u32le": "U32Le",
             "u32be": "U32Be", "u24le": "U24Le", "u24be": "U24Be", "u16le": "U16Le", "u16be": "U16Be", "u8": "U8", "f32le": "F32Le", "f32be": "F32Be",
             "f64le": "F64Le", "f64be": "F64Be", "alaw": "ALaw", "mulaw": "MuLaw"}
IDS = {"s32le": 0x100, "s32be": 0x102, "s24le": 0x104, "s24be": 0x106, "s16le": 0x108, "s16be": 0x10a, "s8": 0x10c, "u32le": 0x10e, "u32be": 0x110,
       "u24le": 0x112, "u24be": 0x114, "u16le": 0x116, "u16be": 0x118, "u8": 0x11a, "f32le": 0x11c, "f32be": 0x11e, "f64le": 0x120, "f64be": 0x122,
       "alaw": 0x124, "mulaw": 0x125}


def harness(dll):
    h = Harness(dll)
    h.it.load_file(ROOT / "tests" / "rust" / "pcm_stubs.rs")
    h.load_shim("ctx.rs", "pcm.rs", "pcmdec.rs")
    r = h.it.call("Context::new", I.Int(0, "i32"))
    assert r.variant == "Ok", r
    return h, r.f["0"]


@pytest.mark.parametrize("make_dll", LIBS)
def test_the_rust_wrapper_decodes_packets(make_dll):
    h, ctx = harness(make_dll())
    rng = np.random.default_rng(9)
    for k, codec in enumerate(R.NAMES):
        cb, nb, fam = R.coded_bytes(codec), R.native_bytes(codec), R.CODECS[codec][3]
        ch, frames = 1 + k % 3, 9 + k
        shift = max(R.legal_shifts(codec)) // 2
        data = rng.integers(0, 256, frames * ch * cb + (cb * ch - 1), dtype=np.uint8)  # a trailing partial frame: dropped
        want = R.decode(data[None, :], codec, ch, frames, shift)
        kind = h.it.resolve_value(["PcmCodec", RUST_NAME[codec]], I.Env(), None)
        assert int(h.it.call_method("PcmCodec", "coded_bytes", kind).v) == cb and int(h.it.call_method("PcmCodec", "native_bytes", kind).v) == nb
        assert int(h.it.call_method("PcmCodec", "raw", kind).v) == k + 1
        found = h.it.call("PcmCodec::from_id", I.Struct("AudioCodecId", {"0": I.Int(IDS[codec], "u32")}))
        assert found.variant == "Some" and found.f["0"].variant == RUST_NAME[codec]
        out = u8_vec(np.full(frames * ch * nb + 3, 0xEE, np.uint8))
        r = h.it.call_method("Context", "pcm_decode", ctx, kind, usize(ch), I.Int(shift, "u32"), u8_vec(data), out)
        assert r.variant == "Ok" and int(r.f["0"].v) == frames, r
        got = np.array([v.v for v in out.a], np.uint8)
        assert np.array_equal(got[:-3], want.view(np.uint8).ravel()) and np.all(got[-3:] == 0xEE), codec
        fmt = h.it.resolve_value(["SampleFormat", "S16"], I.Env(), None)
        out = u8_vec(np.full(frames * ch * 2 + 4, 0xEE, np.uint8))
        r = h.it.call_method("Context", "pcm_decode_as", ctx, kind, usize(ch), I.Int(shift, "u32"), u8_vec(data), fmt, out)
        assert r.variant == "Ok" and int(r.f["0"].v) == frames, r
        got = np.array([v.v for v in out.a], np.uint8)
        assert np.array_equal(got[:-4], R.interleave(want, fam, "s16").ravel()) and np.all(got[-4:] == 0xEE), codec
    # an empty packet and one shorter than a frame are zero frames, not errors
    kind = h.it.resolve_value(["PcmCodec", "S24Be"], I.Env(), None)
    for n in (0, 5):
        r = h.it.call_method("Context", "pcm_decode", ctx, kind, usize(2), I.Int(0, "u32"), u8_vec(np.zeros(n, np.uint8)), u8_vec(np.zeros(0, np.uint8)))
        assert r.variant == "Ok" and int(r.f["0"].v) == 0, r
    # refused shapes go to the decoder below: Unsupported
    for name, ch, shift in (("S16Le", 9, 0), ("S16Le", 2, 16), ("ALaw", 1, 1), ("F32Le", 1, 8)):
        kind = h.it.resolve_value(["PcmCodec", name], I.Env(), None)
        r = h.it.call_method("Context", "pcm_decode", ctx, kind, usize(ch), I.Int(shift, "u32"), u8_vec(np.zeros(72, np.uint8)), u8_vec(np.zeros(288, np.uint8)))
        assert r.variant == "Err" and r.f["0"].variant == "Unsupported", (name, r)
    assert h.it.call("PcmCodec::from_id", I.Struct("AudioCodecId", {"0": I.Int(0x203, "u32")})).variant == "None"  # (ADPCM MS)


def test_the_shim_declares_and_names_the_module():
    sys_rs = (ROOT / "bindings" / "rust" / "symaccel_sys.rs").read_text()
    src = (CRATE / "pcmdec.rs").read_text()
    for name in set(re.findall(r"ffi::(\w+)", src)):
        assert re.search(r"\b%s\b" % name, sys_rs), "%s is not declared in symaccel_sys.rs" % name
    for fn in ("symaccel_pcm_coded_bytes", "symaccel_pcm_native_bytes", "symaccel_pcm_decode", "symaccel_pcm_decode_device", "symaccel_batcher_submit_pcm_decode"):
        assert re.search(r"pub fn %s\(" % fn, sys_rs), fn
    assert re.search(r"SYMACCEL_BATCH_PCM_DECODE: \w+ = 11;", sys_rs) and re.search(r"SYMACCEL_ABI_VERSION: \w+ = 8;", sys_rs)
    lib = (CRATE / "lib.rs").read_text()
    assert "pub mod pcmdec;" in lib
    assert "impl AudioDecoder" not in src  # (the trait impls of the crate's top level are pinned by tests/test_rust_shim.py)


def test_register_still_lists_five():
    lib = (CRATE / "lib.rs").read_text()
    body = lib[lib.index("pub fn register("):]
    body = body[:body.index("\n}\n")]
    assert sorted(re.findall(r"register_one::<(\w+)>", body)) == ["HipAacDecoder", "HipAlacDecoder", "HipFlacDecoder", "HipMpaDecoder", "HipVorbisDecoder"]
    assert "Pcm" not in body and "pcmdec" not in body and "Adpcm" not in body
