"""Packet bytes -> PCM for ADPCM, symphonia-check style (decode the same packets two ways, compare the samples):

  packets of whole blocks (tests/adpcm_writer.py for a synthetic signal, and arbitrary bytes with accepted preambles)
     |
     +--> the REFERENCE: symphonia-codec-adpcm's AdpcmDecoder (lib.rs with codec_ms.rs, codec_ima_wav.rs, codec_ima_qt.rs, common*.rs) on
     |    symphonia-core's own BufReader and packet types, EXECUTED from the reference tree by tools/rsinterp  ..................  PCM_ref
     |
     +--> HipAdpcmDecoder (bindings/rust/symphonia-accel-hip/src/adpcm.rs with decoder.rs, lookahead.rs, ctx.rs, fallback.rs, lib.rs) with
          its extern "C" calls bound to libsymaccel (the CPU-emulation build of the kernels)  ..................................  == PCM_ref

for the three codecs, mono and stereo, several blocks per packet, a block_dur that is no whole number of blocks, trailing bytes and a short
last packet; error packets (a rejected preamble in any block, a packet shorter than its blocks) give the same Error variant, leave the
buffer cleared, and the packets after them decode; behind a LookaheadReader a bad packet inside the look-ahead fails at its own
decode_ref; `adpcm::register` -> `make_audio_decoder` builds decoders that share the cross-stream batcher, no fall-back taken; refused
shapes reach the decoder below.  The three codec files define functions of the same names (decode_mono, read_preamble): each is
registered under its module name, and the QT file's private `read_preamble` is renamed in memory, the interpreter keeping one namespace
for free functions.  Needs the reference tree (`localref`)."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import adpcm_ref as R  # noqa: E402
import adpcm_writer as W  # noqa: E402
from rs_harness import REF, Harness, pool_stats, registry_round_trip, usize  # noqa: E402
from rsinterp import interp as I  # noqa: E402
from rsinterp import parser as P  # noqa: E402

pytestmark = pytest.mark.localref

CRATE = REF / "symphonia-codec-adpcm" / "src"
ID = {"ms": "CODEC_ID_ADPCM_MS", "ima_wav": "CODEC_ID_ADPCM_IMA_WAV", "ima_qt": "CODEC_ID_ADPCM_IMA_QT"}
SHAPES = [("ms", 1, 36, 3), ("ms", 2, 35, 3), ("ima_wav", 1, 41, 2), ("ima_wav", 2, 25, 3), ("ima_qt", 1, 64, 2), ("ima_qt", 2, 64, 2)]  # codec, channels, fpb, blocks per packet
SHAPE_IDS = ["%s_%d" % s[:2] for s in SHAPES]


def load_reference_crate(h):
    it = h.it
    it.load_file(ROOT / "tests" / "rust" / "adpcm_stubs.rs")
    for f in ("common.rs", "common_ima.rs"):
        it.load_file(CRATE / f)
    for mod in ("codec_ms", "codec_ima_wav", "codec_ima_qt"):  # (the QT file last: its decode_stereo calls its own decode_mono unqualified)
        text = (CRATE / (mod + ".rs")).read_text()
        if mod == "codec_ima_qt":
            text = text.replace("read_preamble", "read_preamble_qt")
        it.register_items(P.parse_source(text, mod + ".rs"), mod + ".rs", mod)
    it.load_file(CRATE / "lib.rs")
    assert not it.globals.get("__unparsed__"), it.globals.get("__unparsed__")


def params(h, codec, nch, fpb, max_frames, rate=44100):
    p = h.params(ID[codec], rate=rate, nch=nch)
    p.f["frames_per_block"] = I.some(I.Int(fpb, "u64")) if fpb is not None else I.NONE
    p.f["max_frames_per_packet"] = I.some(I.Int(max_frames, "u64")) if max_frames is not None else I.NONE
    return p


def packet(h, data, pts, dur, track=0, owned=False):
    p = h.packet(data, pts, track=track, owned=owned)
    p.f["dur"] = I.Struct("Duration", {"0": I.Int(int(dur), "u64")})
    return p


def reference(codec, nch, fpb, max_frames):
    h = Harness(None, reference=True, sample="i32")
    load_reference_crate(h)
    r = h.it.call("AdpcmDecoder::try_new", params(h, codec, nch, fpb, max_frames), h.opts())
    assert r.variant == "Ok", r
    return h, r.f["0"]


def shim():
    from emu_lib import emu_library
    h = Harness(emu_library().dll, reference=True, sample="i32")
    h.it.load_file(ROOT / "tests" / "rust" / "adpcm_stubs.rs")
    h.it.load_file(ROOT / "tests" / "rust" / "registry_stubs.rs")
    h.load_shim("lib.rs", "ctx.rs", "decoder.rs", "lookahead.rs", "fallback.rs", "pcm.rs", "adpcm.rs", "adpcm/decoder.rs")
    return h


def hip(h, codec, nch, fpb, max_frames, max_batch=None):
    p = params(h, codec, nch, fpb, max_frames)
    if max_batch is None:
        r = h.it.call("HipAdpcmDecoder::try_registry_new", p, h.opts())  # what the registry calls (registry.rs:34-44)
    else:
        r = h.it.call("HipAdpcmDecoder::try_new", p, h.opts(), usize(max_batch))
    assert r.variant == "Ok", r
    return I.deref(r.f["0"])


def stream(codec, nch, fpb, bpp, n_packets, seed):
    """[(bytes, block_dur)]: encoder packets, then arbitrary bytes; trailing bytes on some, a block_dur with a remainder on some, a short
    last packet -> also the blocks as arrays, for the restatement"""
    rng = np.random.default_rng(seed)
    nb = R.block_bytes(R.CODECS[codec], nch, fpb)
    pcm = W.signal(seed, nch, 2 * bpp * fpb)
    enc = W.encode_ms(pcm, fpb) if codec == "ms" else (W.encode_ima_wav(pcm, fpb) if codec == "ima_wav" else W.encode_ima_qt(pcm))
    out = []
    for i in range(n_packets):
        n = max(1, bpp - 1) if i + 1 == n_packets else bpp
        if i < 2:
            blocks = enc[i * bpp:i * bpp + n]
        else:
            blocks = rng.integers(0, 256, (n, nb), dtype=np.uint8)
            if codec == "ms":
                blocks[:, :nch] %= 7
            elif codec == "ima_wav":
                for c in range(nch):
                    blocks[:, 4 * c + 2] %= 89
        data = blocks.tobytes() + bytes(rng.integers(0, 256, i % 3, dtype=np.uint8))
        out.append((data, n * fpb + (fpb // 2 if i % 2 else 0), blocks))
    return out


def planes_of(blocks, codec, nch, fpb):
    pcm, status = R.decode(blocks, codec, nch, fpb)
    assert not status.any()
    return pcm.transpose(1, 0, 2).reshape(nch, -1)


@pytest.mark.parametrize("codec,nch,fpb,bpp", SHAPES, ids=SHAPE_IDS)
def test_the_accelerated_decoder_equals_the_reference_on_packet_bytes(codec, nch, fpb, bpp):
    packets = stream(codec, nch, fpb, bpp, 5, 3 + nch)
    ref, ref_dec = reference(codec, nch, fpb, bpp * fpb)
    h = shim()
    dec = hip(h, codec, nch, fpb, bpp * fpb, max_batch=1)
    for i, (data, dur, blocks) in enumerate(packets):
        st_r, want = ref.decode("AdpcmDecoder", ref_dec, packet(ref, data, i * bpp * fpb, dur))
        st, got = h.decode("HipAdpcmDecoder", dec, packet(h, data, i * bpp * fpb, dur))
        assert st == st_r == "ok", (i, got, want)
        assert np.array_equal(got, want), i
        assert np.array_equal(want, planes_of(blocks, codec, nch, fpb).astype(np.int64)), i  # (the restatement agrees with both)
    assert h.bridge.calls.count("symaccel_adpcm_decode") == len(packets)  # no look-ahead reader: batches of one
    info = I.deref(h.it.call_method("HipAdpcmDecoder", "codec_info", dec))
    assert info.f["short_name"] == {"ms": "adpcm_ms", "ima_wav": "adpcm_ima_wav", "ima_qt": "adpcm_ima_qt"}[codec]
    h.it.call_method("HipAdpcmDecoder", "finalize", dec)  # (FinalizeResult::default(), as the reference's: nothing to verify)


@pytest.mark.parametrize("codec,nch,fpb,bpp", [s for s in SHAPES if s[0] != "ima_qt"] + [SHAPES[5]], ids=[i for i in SHAPE_IDS if not i.startswith("ima_qt")] + [SHAPE_IDS[5]])
def test_error_packets_fail_like_the_reference_and_the_stream_goes_on(codec, nch, fpb, bpp):
    packets = [list(p[:2]) for p in stream(codec, nch, fpb, bpp, 8, 17)]
    nb = R.block_bytes(R.CODECS[codec], nch, fpb)
    at = (nch - 1) if codec == "ms" else 4 * (nch - 1) + 2
    expect = {}
    if codec != "ima_qt":  # (the QT preamble clamps instead of failing: codec_ima_qt.rs:17)
        for i, block in ((1, 0), (3, bpp - 1)):  # a rejected preamble in the first block of one packet, in the last block of another
            d = bytearray(packets[i][0])
            d[block * nb + at] = 200
            packets[i][0] = bytes(d)
            expect[i] = "Unsupported" if codec == "ms" else "DecodeError"
        d = bytearray(packets[6][0][:(bpp - 1) * nb + at + 1])  # cut inside the last block's preamble, behind a bad byte: the check comes first
        d[(bpp - 1) * nb + at] = 200
        packets[6][0] = bytes(d)
        expect[6] = "Unsupported" if codec == "ms" else "DecodeError"
    packets[4][0] = packets[4][0][:bpp * nb - 1]  # one byte short of its blocks
    expect[4] = "IoError"
    packets[5][0] = packets[5][0][:(bpp - 1) * nb + 1]  # the last block hardly begun
    expect[5] = "IoError"
    ref, ref_dec = reference(codec, nch, fpb, bpp * fpb)
    h = shim()
    dec = hip(h, codec, nch, fpb, bpp * fpb, max_batch=1)
    for i, (data, dur) in enumerate(packets):
        st_r, want = ref.decode("AdpcmDecoder", ref_dec, packet(ref, data, i * bpp * fpb, dur))
        st, got = h.decode("HipAdpcmDecoder", dec, packet(h, data, i * bpp * fpb, dur))  # (decode() checks the buffer is cleared on error)
        assert st == st_r, (i, st, st_r, got, want)
        if i in expect:
            assert (st, got) == ("err", expect[i]) and want == expect[i], (i, got, want)
        else:
            assert st == "ok" and np.array_equal(got, want), i
    assert not h.bridge.calls.count("symaccel_batcher_reserve")  # built without a pool: nothing went to a batcher


def test_look_ahead_batches_a_bad_packet_fails_alone_and_reset():
    """behind a LookaheadReader the packets the demuxer has already read are decoded in ONE device call per batch; a packet with a
    rejected block inside the look-ahead ends the batch in front of it and fails at its own decode_ref; after a seek the application
    resets the decoder and decoding starts over"""
    codec, nch, fpb, bpp = "ms", 2, 35, 3
    packets = [list(p) for p in stream(codec, nch, fpb, bpp, 12, 29)]
    d = bytearray(packets[7][0])
    d[47 + 1] = 9  # the second block's right predictor
    packets[7][0] = bytes(d)
    h = shim()
    dec = hip(h, codec, nch, fpb, bpp * fpb, max_batch=5)
    h.it.load_file(ROOT / "tests" / "rust" / "mocks.rs")
    owned = I.Arr([packet(h, data, i * bpp * fpb, dur, track=1, owned=True) for i, (data, dur, _) in enumerate(packets)], True)
    reader = h.it.call("LookaheadReader::new", h.it.call("MockReader::new", owned), usize(8))

    def run(first, count):
        out = []
        for i in range(first, first + count):
            r = h.it.call_method("LookaheadReader", "next_packet", reader)
            p = r.f["0"].f["0"]
            assert p.f["pts"].f["0"].v == i * bpp * fpb
            out.append(h.decode("HipAdpcmDecoder", dec, h.it.call_method("Packet", "as_packet_ref", p)))
        return out

    n0 = h.bridge.calls.count("symaccel_adpcm_decode")
    for i, (st, got) in enumerate(run(0, 12)):
        if i == 7:
            assert (st, got) == ("err", "Unsupported")
        else:
            assert st == "ok" and np.array_equal(got, planes_of(packets[i][2], codec, nch, fpb)), i
    # packets 0-4 | 5, 6 (the look-ahead stops in front of packet 7) | 7 fails alone, before anything is launched | 8-11
    assert h.bridge.calls.count("symaccel_adpcm_decode") - n0 == 3
    h.it.call_method("LookaheadReader", "seek", reader, I.Int(0, "i64"), usize(3))
    h.it.call_method("HipAdpcmDecoder", "reset", dec)
    for i, (st, got) in zip(range(3, 7), run(3, 4)):
        assert st == "ok" and np.array_equal(got, planes_of(packets[i][2], codec, nch, fpb)), i


def test_decoders_built_by_the_registry_share_the_cross_stream_batcher():
    """`adpcm::register` enters HipAdpcmDecoder at Tier::Preferred, `make_audio_decoder(params, opts)` builds every decoder from (params,
    opts) alone -- and the decoders so built find each other in the process-wide Pool: two streams behind look-ahead readers, decoded
    alternately, every packet's PCM the restatement's (pinned to the reference above), their batches in common launches, no fall-back"""
    codec, nch, fpb, bpp = "ima_wav", 2, 25, 3
    n, depth = 8, 4
    streams = [stream(codec, nch, fpb, bpp, n, 41 + k) for k in range(2)]
    h = shim()
    h.it.load_file(ROOT / "tests" / "rust" / "mocks.rs")
    p = params(h, codec, nch, fpb, bpp * fpb)
    it = h.it
    it.load_file(ROOT / "tests" / "rust" / "registry_generic.rs")
    reg = it.call("CodecRegistry::new")
    it.call("adpcm::register", reg)  # the public entry
    decs = []
    for _ in range(2):
        r = it.call_method("CodecRegistry", "make_registered_audio_decoder", reg, p, h.opts())
        assert r.variant == "Ok", r
        dec = I.deref(r.f["0"])
        assert isinstance(dec, I.Struct) and dec.name == "HipAdpcmDecoder", dec  # no fall-back taken
        decs.append(dec)
    readers = []
    for k, pk in enumerate(streams):
        owned = I.Arr([packet(h, data, i * bpp * fpb, dur, track=1 + k, owned=True) for i, (data, dur, _) in enumerate(pk)], True)
        readers.append(h.it.call("LookaheadReader::new", h.it.call("MockReader::new", owned), usize(depth)))
    for i in range(n):
        for k in range(2):
            r = h.it.call_method("LookaheadReader", "next_packet", readers[k])
            st, got = h.decode("HipAdpcmDecoder", decs[k], h.it.call_method("Packet", "as_packet_ref", r.f["0"].f["0"]))
            assert st == "ok" and np.array_equal(got, planes_of(streams[k][i][2], codec, nch, fpb)), (k, i)
    calls = h.bridge.calls
    assert calls.count("symaccel_batcher_create") == 1 and calls.count("symaccel_batcher_reserve") >= 2
    assert calls.count("symaccel_adpcm_decode") == 2  # each stream's cold start only: every later batch went through the batcher
    stats = pool_stats(h)
    assert stats["submissions"] >= 2 and stats["launches"] < stats["submissions"] and stats["failed_tickets"] == 0, stats


def test_refused_shapes_and_missing_parameters_reach_the_decoder_below():
    """a shape the device decoder refuses is handed to the factory that was registered below (here: a stand-in that records the call);
    without one the reason comes back as Unsupported, as the reference's try_new reports its own refusals"""
    h = shim()
    it = h.it
    for codec, nch, fpb, max_frames in (("ms", 1, 35, 70), ("ima_wav", 1, 40, 80), ("ima_wav", 2, 10, 40), ("ima_qt", 2, 32, 64), ("ms", 2, None, 64), ("ms", 2, 35, None),
                                        ("ms", 2, 0, 64)):
        r = it.call("HipAdpcmDecoder::try_new", params(h, codec, nch, fpb, max_frames), h.opts(), usize(4))
        assert r.variant == "Err" and r.f["0"].variant == "Unsupported", (codec, nch, fpb, r)
        r = it.call("HipAdpcmDecoder::try_registry_new", params(h, codec, nch, fpb, max_frames), h.opts())  # nothing below: the reason
        assert r.variant == "Err" and r.f["0"].variant == "Unsupported", (codec, nch, fpb, r)
    r = it.call("HipAdpcmDecoder::try_new", params(h, "ms", 2, 35, 70, rate=None), h.opts(), usize(4))
    assert r.variant == "Err" and r.f["0"].variant == "Unsupported"
    # with a decoder below: registered first, then adpcm::register above it; a refused shape gets the one below, an accepted one ours
    it.load_file(ROOT / "tests" / "rust" / "registry_generic.rs")
    it.load_source("""
pub struct BelowDecoder { pub params: AudioCodecParameters }
impl RegisterableAudioDecoder for BelowDecoder {
    fn try_registry_new(params: &AudioCodecParameters, _opts: &AudioDecoderOptions) -> Result<Box<dyn AudioDecoder>> { Ok(Box::new(BelowDecoder { params: params.clone() })) }
    fn supported_codecs() -> &'static [SupportedAudioCodec] { &[support_audio_codec!(CODEC_ID_ADPCM_IMA_WAV, "below", "the decoder below")] }
}
pub fn register_below(registry: &mut CodecRegistry) { registry.register_audio_decoder_at_tier::<BelowDecoder>(Tier::Standard); }
""", "below.rs")
    reg = it.call("CodecRegistry::new")
    it.call("register_below", reg)
    it.call("adpcm::register", reg)
    r = it.call_method("CodecRegistry", "make_registered_audio_decoder", reg, params(h, "ima_wav", 2, 10, 40), h.opts())
    assert r.variant == "Ok" and I.deref(r.f["0"]).name == "BelowDecoder", r
    r = it.call_method("CodecRegistry", "make_registered_audio_decoder", reg, params(h, "ima_wav", 2, 25, 75), h.opts())
    assert r.variant == "Ok" and I.deref(r.f["0"]).name == "HipAdpcmDecoder", r


def test_the_adapter_implements_the_traits_as_the_reference_states_them():
    """tests/test_rust_shim.py checks the crate's top-level files; the adapter lives in src/adpcm/decoder.rs: the same comparison of its
    `impl AudioDecoder` / `impl RegisterableAudioDecoder` with the trait text of the reference, method by method"""
    import test_rust_shim as S
    seen = []
    for it in S.expanded_items(S.CRATE / "adpcm" / "decoder.rs"):
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
    assert sorted(seen) == [("AudioDecoder", "HipAdpcmDecoder"), ("RegisterableAudioDecoder", "HipAdpcmDecoder")]


@pytest.mark.parametrize("expr,want", [("Some(3u64).is_none_or(|v| v == 0)", False), ("Some(0u64).is_none_or(|v| v == 0)", True),
                                       ("None::<u64>.is_none_or(|v| v == 0)", True), ("Some(3u64).is_some_and(|v| v == 3)", True),
                                       ("None::<u64>.is_some_and(|v| v == 3)", False)])
def test_interpreter_option_predicates(expr, want):
    """std: Option::is_none_or is true for None and otherwise the predicate of the value (lib.rs:84 uses it); is_some_and is false for
    None.  Expectations from the std documentation, not read off the interpreter."""
    from rsinterp import Interp
    it = Interp()
    it.load_source("pub fn probe() -> bool {\n%s\n}\n" % expr, "probe.rs")
    assert bool(it.call("probe")) is want and it.overflows == 0
