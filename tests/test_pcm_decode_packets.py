"""Packet bytes -> PCM for PCM / G.711, symphonia-check style (decode the same packets two ways, compare the samples):

  written packets (a long one, a short one after it, an empty one, one frame, a trailing partial frame, less than a frame, one above
  max_frames_per_packet, one below it again)
     |
     +--> the REFERENCE: symphonia-codec-pcm's PcmDecoder (lib.rs) on symphonia-core's own io/, packet.rs, audio/sample.rs and
     |    audio/conv.rs, EXECUTED from the reference tree by tools/rsinterp (tools/make_pcm_decode_fixtures.py: decoder_harness, with
     |    the container stand-ins and the one in-memory rewrite it states)  ............................................  planes_ref
     |
     +--> HipPcmDecoder (bindings/rust/symphonia-accel-hip/src/pcmdec.rs with pcmdec/decoder.rs, lookahead.rs, ctx.rs, fallback.rs,
          lib.rs) with its extern "C" calls bound to libsymaccel (the CPU-emulation build of the kernels)  ...............  == planes_ref

for all 20 codecs: equal frame counts, equal planes (floats as bits) and the same buffer variant; behind look-ahead readers the packets
of a batch -- of different lengths, the empty ones included -- go to the device in one call; `pcmdec::register` ->
`make_audio_decoder` builds decoders that share the cross-stream batcher, no fall-back taken (the batcher's statistics); refused shapes
reach the decoder below; `try_new` refuses what the reference's refuses, with its variants (the fixture's recorded refusals and the
reference itself).  Needs the reference tree (`localref`)."""
import json
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import make_pcm_decode_fixtures as M  # noqa: E402
import pcm_decode_ref as R  # noqa: E402
from rs_harness import REF, Harness, pool_stats, usize  # noqa: E402
from rsinterp import interp as I  # noqa: E402

pytestmark = pytest.mark.localref

MAX_FRAMES = 12


def shim():
    from emu_lib import emu_library
    h = Harness(emu_library().dll, reference=True, sample="i32")
    h.it.load_file(ROOT / "tests" / "rust" / "pcm_stubs.rs")
    h.it.load_file(ROOT / "tests" / "rust" / "registry_stubs.rs")
    h.load_shim("lib.rs", "ctx.rs", "decoder.rs", "lookahead.rs", "fallback.rs", "pcm.rs", "pcmdec.rs", "pcmdec/decoder.rs")
    # (behind the shim: the interpreter keeps one namespace for types, and symphonia-core's SampleFormat -- the one decoder.rs imports, a
    # superset of the crate's own pcm::SampleFormat, whose methods stay -- must be the one `SampleFormat::F64` resolves in)
    for f in ("audio/sample.rs", "audio/conv.rs"):
        h.it.load_file(REF / "symphonia-core" / "src" / f)
    return h


def codec_id(codec):
    return "CODEC_ID_PCM_" + codec.upper()


def hip(h, codec, nch, shift=0, max_batch=None, max_frames=MAX_FRAMES):
    w = R.WIDTH[R.CODECS[codec][3]]
    p = M.pcm_params(h, codec_id(codec), 8000, nch, w if shift else None, w - shift if shift else None, max_frames)
    if max_batch is None:
        r = h.it.call("HipPcmDecoder::try_registry_new", p, h.opts())  # what the registry calls (registry.rs:34-44)
    else:
        r = h.it.call("HipPcmDecoder::try_new", p, h.opts(), usize(max_batch))
    assert r.variant == "Ok", r
    return I.deref(r.f["0"])


def reference(ref, codec, nch, shift=0):
    w = R.WIDTH[R.CODECS[codec][3]]
    r = ref.it.call("PcmDecoder::try_new", M.pcm_params(ref, codec_id(codec), 8000, nch, w if shift else None, w - shift if shift else None, MAX_FRAMES), ref.opts())
    assert r.variant == "Ok", r
    return r.f["0"]


def decode(h, type_name, dec, pkt):
    """decode_ref -> (buffer variant, frames, planes as integers / float bits [channel][frame]); last_decoded() is the same buffer"""
    r = h.it.call_method(type_name, "decode_ref", dec, pkt)
    assert r.variant == "Ok", r  # no packet can fail (lib.rs:328)
    g = I.deref(r.f["0"])
    buf = I.deref(g.f["0"])
    assert I.deref(I.deref(h.it.call_method(type_name, "last_decoded", dec)).f["0"]) is buf
    frames = int(I.deref(buf.f["num_frames"]).v)
    planes = [[M.sample_bits(v, None) for v in I.deref(pl).a[:frames]] for pl in I.deref(buf.f["planes"]).a]
    return g.variant, frames, planes


def written_packets(codec, nch, seed):
    fb = R.coded_bytes(codec) * nch
    rng = np.random.default_rng(seed)
    lens = [9 * fb, 4 * fb, 0, fb, 5 * fb + fb - 1, fb - 1 if fb > 1 else 0, (MAX_FRAMES + 3) * fb, 2 * fb]
    return [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]


_REF_H = {"h": None}


def ref_harness():
    if _REF_H["h"] is None:
        _REF_H["h"] = M.decoder_harness()
    return _REF_H["h"]


@pytest.fixture(scope="module")
def shim_h():
    return shim()


@pytest.mark.parametrize("codec", R.NAMES)
def test_the_accelerated_decoder_equals_the_reference_on_packet_bytes(shim_h, codec):
    k = R.NAMES.index(codec)
    nch = (1, 2, 3, 8)[k % 4] if codec not in ("s24le", "s24be") else 3
    kind, fam = R.CODECS[codec][1], R.CODECS[codec][3]
    shift = (R.WIDTH[fam] // 2 + 1) if kind in "su" and k % 2 else 0
    ref, h = ref_harness(), shim_h
    ref_dec = reference(ref, codec, nch, shift)
    dec = hip(h, codec, nch, shift, max_batch=1)
    n0 = h.bridge.calls.count("symaccel_pcm_decode")
    packets = written_packets(codec, nch, 100 + k)
    for i, data in enumerate(packets):
        want = decode(ref, "PcmDecoder", ref_dec, ref.packet(data, i))
        got = decode(h, "HipPcmDecoder", dec, h.packet(data, i))
        assert got[0] == want[0] == fam.upper() and got[1] == want[1] == R.frames_of(len(data), codec, nch), (codec, i, got[:2], want[:2])
        assert got[2] == want[2], (codec, i)
    # no look-ahead reader: batches of one; a packet without a whole frame launches nothing
    assert h.bridge.calls.count("symaccel_pcm_decode") - n0 == sum(1 for d in packets if R.frames_of(len(d), codec, nch))
    info = I.deref(h.it.call_method("HipPcmDecoder", "codec_info", dec))
    ref_info = I.deref(ref.it.call_method("PcmDecoder", "codec_info", ref_dec))
    assert info.f["short_name"] == ref_info.f["short_name"] == "pcm_" + codec
    h.it.call_method("HipPcmDecoder", "finalize", dec)
    h.it.call_method("HipPcmDecoder", "reset", dec)  # (does nothing: lib.rs:415-417)
    assert decode(h, "HipPcmDecoder", dec, h.packet(packets[0], 99))[2] == decode(ref, "PcmDecoder", ref_dec, ref.packet(packets[0], 99))[2]


def test_decoders_built_by_the_registry_share_the_cross_stream_batcher():
    """`pcmdec::register` enters HipPcmDecoder at Tier::Preferred, `make_audio_decoder(params, opts)` builds every decoder from (params,
    opts) alone -- and the decoders so built find each other in the process-wide Pool: two streams behind look-ahead readers, decoded
    alternately, every packet's planes the restatement's (pinned to the reference above and in tests/test_pcm_decode.py), their batches in
    common launches, no fall-back"""
    codec, nch = "s24be", 2
    n, depth = 8, 4
    fb = R.coded_bytes(codec) * nch
    rng = np.random.default_rng(7)
    streams = [[rng.integers(0, 256, (10 if i + 1 < n else 3) * fb + (i % 3), dtype=np.uint8) for i in range(n)] for _ in range(2)]
    h = shim()
    it = h.it
    it.load_file(ROOT / "tests" / "rust" / "mocks.rs")
    it.load_file(ROOT / "tests" / "rust" / "registry_generic.rs")
    p = M.pcm_params(h, codec_id(codec), 8000, nch, None, None, 10)
    reg = it.call("CodecRegistry::new")
    it.call("pcmdec::register", reg)  # the public entry
    decs = []
    for _ in range(2):
        r = it.call_method("CodecRegistry", "make_registered_audio_decoder", reg, p, h.opts())
        assert r.variant == "Ok", r
        dec = I.deref(r.f["0"])
        assert isinstance(dec, I.Struct) and dec.name == "HipPcmDecoder", dec  # no fall-back taken
        decs.append(dec)
    readers = []
    for k, pk in enumerate(streams):
        owned = I.Arr([h.packet(data, i * 10, track=1 + k, owned=True) for i, data in enumerate(pk)], True)
        readers.append(it.call("LookaheadReader::new", it.call("MockReader::new", owned), usize(depth)))
    for i in range(n):
        for k in range(2):
            r = it.call_method("LookaheadReader", "next_packet", readers[k])
            variant, frames, planes = decode(h, "HipPcmDecoder", decs[k], it.call_method("Packet", "as_packet_ref", r.f["0"].f["0"]))
            want = R.decode(streams[k][i][None, :], codec, nch, R.frames_of(len(streams[k][i]), codec, nch))[0]
            assert variant == "S24" and frames == want.shape[1] and np.array_equal(np.array(planes, np.int64).reshape(nch, frames), want.astype(np.int64)), (k, i)
    calls = h.bridge.calls
    assert calls.count("symaccel_batcher_create") == 1 and calls.count("symaccel_batcher_reserve") >= 2
    assert calls.count("symaccel_pcm_decode") == 2  # each stream's cold start only: every later batch went through the batcher
    stats = pool_stats(h)
    assert stats["submissions"] >= 2 and stats["launches"] < stats["submissions"] and stats["failed_tickets"] == 0, stats


def test_try_new_refuses_what_the_reference_refuses_with_its_variants():
    z = np.load(ROOT / "tests" / "golden" / "pcm_decode.npz")
    recorded = json.loads(bytes(z["manifest"]).decode())["try_new_refusals"]
    assert len(recorded) == 13
    h, ref = shim(), ref_harness()
    for r in recorded + [{"codec": "CODEC_ID_PCM_S16LE", "sample_rate": 8000, "channels": 0, "bits_per_sample": None, "bits_per_coded_sample": None,
                          "error": "Unsupported", "message": "pcm: number of channels cannot be 0"}]:
        args = (r["codec"], r["sample_rate"], r["channels"], r["bits_per_sample"], r["bits_per_coded_sample"], None)
        want = ref.it.call("PcmDecoder::try_new", M.pcm_params(ref, *args), ref.opts())
        pr = M.pcm_params(h, *args)
        if r["channels"] == 0:  # (the harness writes no channels for 0: an empty layout is meant)
            pr.f["channels"] = I.some(I.Enum("Channels", "Discrete", {"0": I.Int(0, "u16")}))
            want = ref.it.call("PcmDecoder::try_new", pr, ref.opts())
        got = h.it.call("HipPcmDecoder::try_new", pr, h.opts(), usize(4))
        assert got.variant == want.variant == "Err", r
        ge, we = I.deref(got.f["0"]), I.deref(want.f["0"])
        assert ge.variant == we.variant == r["error"], (r, ge.variant, we.variant)
        assert str(I.deref(ge.f["0"])) == str(I.deref(we.f["0"])) == r["message"], r


def test_refused_shapes_reach_the_decoder_below():
    """a shape the device decoder refuses (nine channels; a coded width of 0) is handed to the factory that was registered below (here:
    a stand-in that records the call); without one the reason comes back as Unsupported"""
    h = shim()
    it = h.it
    nine = M.pcm_params(h, "CODEC_ID_PCM_S16LE", 8000, 9, None, None, None)
    zero_width = M.pcm_params(h, "CODEC_ID_PCM_S16LE", 8000, 2, 16, None, None)
    zero_width.f["bits_per_coded_sample"] = I.some(I.Int(0, "u32"))
    for p in (nine, zero_width):
        r = it.call("HipPcmDecoder::try_new", p, h.opts(), usize(4))
        assert r.variant == "Err" and I.deref(r.f["0"]).variant == "Unsupported", r
        r = it.call("HipPcmDecoder::try_registry_new", p, h.opts())  # nothing below: the reason
        assert r.variant == "Err" and I.deref(r.f["0"]).variant == "Unsupported", r
    it.load_file(ROOT / "tests" / "rust" / "registry_generic.rs")
    it.load_source("""
pub struct BelowDecoder { pub params: AudioCodecParameters }
impl RegisterableAudioDecoder for BelowDecoder {
    fn try_registry_new(params: &AudioCodecParameters, _opts: &AudioDecoderOptions) -> Result<Box<dyn AudioDecoder>> { Ok(Box::new(BelowDecoder { params: params.clone() })) }
    fn supported_codecs() -> &'static [SupportedAudioCodec] { &[support_audio_codec!(CODEC_ID_PCM_S16LE, "below", "the decoder below")] }
}
pub fn register_below(registry: &mut CodecRegistry) { registry.register_audio_decoder_at_tier::<BelowDecoder>(Tier::Standard); }
""", "below.rs")
    reg = it.call("CodecRegistry::new")
    it.call("register_below", reg)
    it.call("pcmdec::register", reg)
    r = it.call_method("CodecRegistry", "make_registered_audio_decoder", reg, nine, h.opts())
    assert r.variant == "Ok" and I.deref(r.f["0"]).name == "BelowDecoder", r
    r = it.call_method("CodecRegistry", "make_registered_audio_decoder", reg, M.pcm_params(h, "CODEC_ID_PCM_S16LE", 8000, 2, None, None, None), h.opts())
    assert r.variant == "Ok" and I.deref(r.f["0"]).name == "HipPcmDecoder", r


def test_the_adapter_implements_the_traits_as_the_reference_states_them():
    """tests/test_rust_shim.py checks the crate's top-level files; the adapter lives in src/pcmdec/decoder.rs: the same comparison of its
    `impl AudioDecoder` / `impl RegisterableAudioDecoder` with the trait text of the reference, method by method; all twenty ids entered"""
    import test_rust_shim as S
    seen = []
    for it in S.expanded_items(S.CRATE / "pcmdec" / "decoder.rs"):
        if it[0] != "impl" or it[2] is None or it[2][0] != "tpath" or it[2][1][-1] not in ("AudioDecoder", "RegisterableAudioDecoder"):
            continue
        want = S.trait_methods(it[2][1][-1])
        have = {m[1]: m for m in it[3] if m[0] == "fn"}
        assert not set(have) - set(want) and not {n for n, m in want.items() if m[6] is None} - set(have), (sorted(have), sorted(want))
        for n, m in have.items():
            w = want[n]
            assert m[4] == w[4] and len(m[3]) == len(w[3]), n
            assert [S.type_shape(t) for _, t in m[3]] == [S.type_shape(t) for _, t in w[3]] and S.type_shape(m[5]) == S.type_shape(w[5]), n
        seen.append((it[2][1][-1], S.type_shape(it[1])))
    assert sorted(seen) == [("AudioDecoder", "HipPcmDecoder"), ("RegisterableAudioDecoder", "HipPcmDecoder")]
    text = (S.CRATE / "pcmdec" / "decoder.rs").read_text()
    assert sorted(set(__import__("re").findall(r"support_audio_codec!\((CODEC_ID_PCM_\w+),", text))) == sorted(codec_id(c) for c in R.NAMES)
