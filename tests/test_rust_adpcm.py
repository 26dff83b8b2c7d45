"""The Rust side of the ADPCM decode, EXECUTED: bindings/rust/symphonia-accel-hip/src/adpcm.rs (`AdpcmCodec`, `Context::adpcm_decode`,
`Context::adpcm_decode_as`) under tools/rsinterp with its `extern "C"` calls bound to libsymaccel (the CPU-emulation build here, the
hipcc-built library in the gpu twin), against the numpy restatement of tests/adpcm_ref.py (pinned to the reference fixture by
tests/test_adpcm.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import adpcm_ref as R  # noqa: E402
from rs_harness import Harness, i32_vec, u8_vec, usize  # noqa: E402
from rsinterp import interp as I  # noqa: E402
from test_rust_adapters import LIBS  # noqa: E402

RUST_NAME = {"ms": "Ms", "ima_wav": "ImaWav", "ima_qt": "ImaQt"}


@pytest.mark.parametrize("make_dll", LIBS)
def test_the_rust_wrapper_decodes_blocks(make_dll):
    h = Harness(make_dll())
    h.load_shim("ctx.rs", "pcm.rs", "adpcm.rs")  # (the context-level call; the decoder of src/adpcm/decoder.rs: tests/test_adpcm_packets.py)
    r = h.it.call("Context::new", I.Int(0, "i32"))
    assert r.variant == "Ok", r
    ctx = r.f["0"]
    rng = np.random.default_rng(9)
    for codec, ch, fpb, n in (("ms", 2, 35, 3), ("ms", 1, 20, 2), ("ima_wav", 1, 41, 3), ("ima_wav", 2, 17, 2), ("ima_qt", 2, 64, 2)):
        nb = R.block_bytes(R.CODECS[codec], ch, fpb)
        blocks = rng.integers(0, 256, (n, nb), dtype=np.uint8)
        if codec == "ms":
            blocks[:, :ch] %= 7
            blocks[1, 0] = 7  # a block the reference rejects
        elif codec == "ima_wav":
            blocks[:, 2] %= 89
            blocks[:, 6 % nb] %= 89
            blocks[1, 2] = 99
        want, want_status = R.decode(blocks, codec, ch, fpb)
        kind = h.it.resolve_value(["AdpcmCodec", RUST_NAME[codec]], I.Env(), None)
        got_bytes = h.it.call_method("AdpcmCodec", "block_bytes", kind, usize(ch), usize(fpb))
        assert got_bytes.variant == "Some" and int(got_bytes.f["0"].v) == nb
        pcm, status = i32_vec(np.full(n * ch * fpb + 3, 77, np.int32)), u8_vec(np.full(n + 2, 0xEE, np.uint8))
        r = h.it.call_method("Context", "adpcm_decode", ctx, kind, usize(ch), usize(fpb), u8_vec(blocks.ravel()), pcm, status)
        assert r.variant == "Ok", r
        got = np.array([v.v for v in pcm.a], np.int64).astype(np.int32)
        assert np.array_equal(got[:-3].reshape(n, ch, fpb), want) and np.all(got[-3:] == 77), codec
        st = np.array([v.v for v in status.a], np.uint8)
        assert np.array_equal(st[:n], want_status) and np.all(st[n:] == 0xEE)
        fmt = h.it.resolve_value(["SampleFormat", "S16"], I.Env(), None)
        out = u8_vec(np.full(n * ch * fpb * 2 + 4, 0xEE, np.uint8))
        r = h.it.call_method("Context", "adpcm_decode_as", ctx, kind, usize(ch), usize(fpb), u8_vec(blocks.ravel()), fmt, out, status)
        assert r.variant == "Ok", r
        got16 = np.array([v.v for v in out.a], np.uint8)
        assert np.array_equal(got16[:-4].view(np.int16).reshape(n, fpb, ch), (want >> 16).astype(np.int16).transpose(0, 2, 1)) and np.all(got16[-4:] == 0xEE)
    # no blocks is nothing to do, not an error
    kind = h.it.resolve_value(["AdpcmCodec", "Ms"], I.Env(), None)
    r = h.it.call_method("Context", "adpcm_decode", ctx, kind, usize(2), usize(35), u8_vec(np.zeros(0, np.uint8)), i32_vec(np.zeros(0, np.int32)), u8_vec(np.zeros(0, np.uint8)))
    assert r.variant == "Ok", r
    # refused shapes: no block size, and the call is Unsupported
    kind = h.it.resolve_value(["AdpcmCodec", "ImaWav"], I.Env(), None)
    assert h.it.call_method("AdpcmCodec", "block_bytes", kind, usize(2), usize(10)).variant == "None"
    r = h.it.call_method("Context", "adpcm_decode", ctx, kind, usize(2), usize(10), u8_vec(np.zeros(17, np.uint8)), i32_vec(np.zeros(20, np.int32)), u8_vec(np.zeros(1, np.uint8)))
    assert r.variant == "Err" and r.f["0"].variant == "Unsupported", r
