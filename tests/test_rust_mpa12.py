"""The Rust side of the Layer I / II decode, EXECUTED: bindings/rust/symphonia-accel-hip/src/mpa12.rs (`MpaLayer`, `Context::mpa12_decode`)
under tools/rsinterp with its `extern "C"` calls bound to libsymaccel (the CPU-emulation build here, the hipcc-built library in the gpu
twin), against tests/mpa12_ref.py + the oracle's polyphase (pinned to the interpreted reference by tests/test_mpa12.py); and the
module's shape: it parses, is a public module of the crate, and calls the generated declaration with its arguments in order."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import mpa12_ref as R  # noqa: E402
from helpers import bit_equal  # noqa: E402
from rs_harness import CRATE, Harness, f32_vec, i32_vec, u8_vec, usize  # noqa: E402
from rsinterp import interp as I  # noqa: E402
from rsinterp import parser as P  # noqa: E402
from test_mpa12 import case  # noqa: E402
from test_rust_adapters import LIBS  # noqa: E402


def u16_vec(a):
    return I.Arr([I.Int(int(x), "u16") for x in np.asarray(a).ravel()], True)


def floats(arr):
    return np.array([np.float32(x) if not isinstance(x, I.Int) else np.float32(x.v) for x in arr.a], np.float32)


def test_the_module_parses_and_binds_the_generated_declaration():
    src = (CRATE / "mpa12.rs").read_text()
    items = P.parse_source(src, "mpa12.rs")
    assert not [it for it in items if it[0] == "unparsed"]
    assert {it[1] for it in items if it[0] == "enum"} == {"MpaLayer"}
    assert re.search(r"^pub mod mpa12;", (CRATE / "lib.rs").read_text(), flags=re.M) and "pub use mpa12::{HipMpa12Decoder, MpaLayer};" in (CRATE / "lib.rs").read_text()
    decl = re.search(r"pub fn symaccel_mpa12_decode\(([^)]*)\) -> i32;", (ROOT / "bindings/rust/symaccel_sys.rs").read_text()).group(1)
    names = [a.split(":")[0].strip() for a in decl.split(",")]
    assert names == ["ctx", "layer", "h_codes", "h_rec", "h_vvec_io", "h_vfront_io", "h_pcm", "h_status", "n_chains", "packets_per_chain"]
    call = re.search(r"ffi::symaccel_mpa12_decode\(([^;]*)\)\s*\n\s*\};", src).group(1)
    args = [a.strip() for a in re.sub(r"\s+", " ", call).split(", ")]
    assert args == ["self.raw()", "layer.raw()", "codes.as_ptr()", "rec.as_ptr()", "vvec.as_mut_ptr()", "vfront.as_mut_ptr()", "pcm.as_mut_ptr()", "status.as_mut_ptr()",
                    "n_chains", "packets"]


def impls_of(path):
    """{(trait or None, type): {method: item}} of a crate file, what its `hip_decoder!` invocation expands to included"""
    from test_rust_shim import expanded_items
    out = {}
    for it in expanded_items(path):
        if it[0] == "impl":
            out.setdefault((it[2][1][-1] if it[2] is not None else None, it[1][1][-1]), {}).update({m[1]: m for m in it[3] if m[0] == "fn"})
    return out


def test_the_decoder_module_has_the_traits_and_the_calls():
    """src/mpa12/decoder.rs: it parses down to every function body, what `hip_decoder!` (decoder.rs) makes of its invocation included;
    `HipMpa12Decoder` implements `AudioDecoder` and `RegisterableAudioDecoder` in the SUBMODULE (mpa12.rs has no impl of either),
    `Mpa12Batch` the crate's `BatchCodec`; `register` enters it through `register_one`, `register()` of lib.rs keeps its five; the front
    end is the patched decoder with the recorder; the library is reached through `symaccel_mpa12_decode` and batcher kind 10 (through
    the slot cycle of ctx.rs); a decoder that cannot be built goes to the one below"""
    from test_rust_shim import expanded_items
    path = CRATE / "mpa12" / "decoder.rs"
    src = path.read_text()
    items = expanded_items(path)
    assert not [it for it in items if it[0] in ("unparsed", "macro_item")]
    for it in items:
        if it[0] == "impl":
            for m in it[3]:
                if m[0] == "fn" and m[6] is not None:
                    m[8].parse_body(m[6])
    impls = impls_of(path)
    assert set(impls[("AudioDecoder", "HipMpa12Decoder")]) == {"reset", "codec_info", "codec_params", "decode_ref", "finalize", "last_decoded"}
    assert set(impls[("RegisterableAudioDecoder", "HipMpa12Decoder")]) == {"try_registry_new", "supported_codecs"}
    assert {"parse", "transform", "publish", "reset_state", "clear", "pooled", "submit", "collect", "hint", "abandon"} <= set(impls[("BatchCodec", "Mpa12Batch")])
    assert set(impls[("SubbandBackend", "SubbandRecorder")]) == {"decode_frame", "reset"}
    assert not any(k[0] in ("AudioDecoder", "RegisterableAudioDecoder") for k in impls_of(CRATE / "mpa12.rs"))
    assert "crate::register_one::<HipMpa12Decoder>(registry, true);" in src and "CODEC_ID_MP1" in src and "CODEC_ID_MP2" in src
    assert "MpaDecoder::try_new_with_subband_backend(params, &front_opts, Box::new(SubbandRecorder(record.clone())))" in src
    assert "ffi::symaccel_mpa12_decode(" in src and "ffi::SYMACCEL_BATCH_MPA12_DECODE as i32, self.layer.raw(), nch, k" in src
    assert "self.slots.submit(ffi::SYMACCEL_BATCH_MPA12_DECODE as i32" in src and "self.slots.out::<f32>()" in src
    assert "self.buf.trim(trims[i].0, trims[i].1);" in src and "crate::fallback::make(params, opts, e)" in (CRATE / "decoder.rs").read_text()
    try_registry_new = impls[("RegisterableAudioDecoder", "HipMpa12Decoder")]["try_registry_new"]
    assert "fallback" in repr(try_registry_new[8].parse_body(try_registry_new[6]))
    lib = (CRATE / "lib.rs").read_text()
    assert lib.count("register_one::<Hip") == 5 and "HipMpa12Decoder>(registry" not in lib
    assert 'features = ["mp1", "mp2", "mp3"]' in (CRATE.parent / "Cargo.toml").read_text()


@pytest.mark.localref
def test_the_recorder_implements_the_patched_trait():
    """method names, receivers and parameter shapes of `impl SubbandBackend for SubbandRecorder` == the trait of the patched crate"""
    from rs_harness import patched_tree
    from test_rust_shim import type_shape
    tree = patched_tree(("symphonia-bundle-mp3",))
    trait = next(it for it in P.parse_source((tree / "symphonia-bundle-mp3/src/backend.rs").read_text(), "backend.rs") if it[0] == "trait" and it[1] == "SubbandBackend")
    want = {m[1]: m for m in trait[2] if m[0] == "fn"}
    have = impls_of(CRATE / "mpa12" / "decoder.rs")[("SubbandBackend", "SubbandRecorder")]
    assert set(have) == set(want)
    for n, m in have.items():
        assert m[4] == want[n][4] == "ref_mut" and len(m[3]) == len(want[n][3]), n
        for (_, ta), (_, tb) in zip(m[3], want[n][3]):
            assert type_shape(ta) == type_shape(tb), (n, type_shape(ta), type_shape(tb))


@pytest.mark.parametrize("make_dll", LIBS)
def test_the_rust_wrapper_decodes_packets(make_dll):
    h = Harness(make_dll())
    h.load_shim("ctx.rs", "mpa12.rs")
    r = h.it.call("Context::new", I.Int(0, "i32"))
    assert r.variant == "Ok", r
    ctx = r.f["0"]
    for layer, name, nch, npk in ((R.LAYER1, "Layer1", 2, 2), (R.LAYER2, "Layer2", 1, 1)):
        (codes, rec, vvec, vfront), want = case(layer, nch, npk)
        rec = rec.copy()
        if layer == R.LAYER1:
            rec[1, 1, 3] = 1  # a record out of range: status 1, that channel-packet alone is silence
            want = R.decode(layer, codes, rec, vvec, vfront)
        kind = h.it.resolve_value(["MpaLayer", name], I.Env(), None)
        assert int(h.it.call_method("MpaLayer", "record_bytes", kind).v) == R.RECORD_BYTES[layer]
        assert int(h.it.call_method("MpaLayer", "n_frames", kind).v) == R.N_FRAMES[layer]
        vv, vf = f32_vec(vvec), i32_vec(vfront)
        pcm, status = f32_vec(np.full(want[0].size + 2, 5.0, np.float32)), u8_vec(np.full(nch * npk + 1, 0xEE, np.uint8))
        r = h.it.call_method("Context", "mpa12_decode", ctx, kind, usize(nch), u16_vec(codes), u8_vec(rec.ravel()), vv, vf, pcm, status)
        assert r.variant == "Ok", r
        got = floats(pcm)
        assert bit_equal(got[:-2].reshape(want[0].shape), want[0]) and np.all(got[-2:] == 5.0), name
        assert bit_equal(floats(vv).reshape(nch, 1024), want[1]) and np.array_equal(np.array([v.v for v in vf.a], np.int32), want[2])
        st = np.array([v.v for v in status.a], np.uint8)
        assert np.array_equal(st[:-1].reshape(nch, npk), want[3]) and st[-1] == 0xEE
