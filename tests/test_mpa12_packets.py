"""Written Layer I / II packets through the reference's own `Layer1::decode` / `Layer2::decode` under tools/rsinterp (needs the reference
tree: `localref`) against the library fed what the writer put into the packets (tests/mpa12_writer.py), on the emulation build:

  * tests/golden/mpa12 regenerates from the reference tree, array for array;
  * a packet the reference refuses -- a Layer I allocation of 15 ("mp1: invalid bit allocation"), a packet whose reads run out -- fails
    alone, contributes no unit and leaves the SynthesisState untouched: the packets around it decode to what the library makes of them as
    CONSECUTIVE units, bit for bit, and the reference's state after the run is the library's.

  * the seam (bindings/rust/patches/symphonia-bundle-mp3.diff, `SubbandBackend`): the PATCHED `Layer1` / `Layer2` without a backend
    decode the fixture packets to the unpatched decoders' PCM, bit for bit; with a recording backend (tests/rust/mpa12_stubs.rs) what
    crosses the seam is exactly what the writer put into the packets -- the codes and records symaccel_mpa12_decode takes --, no PCM
    is computed on the host and the decoder's own filterbank state stays untouched.

  * three decoders on written packets: the reference's unpatched `MpaDecoder`, its patched twin without a backend and `HipMpa12Decoder`
    (bindings/rust/symphonia-accel-hip/src/mpa12/decoder.rs: the patched decoder with a recording backend as front end, the emulation
    library behind it) agree bit for bit -- across look-ahead batch boundaries, with a damaged packet in mid-batch (the same error, the
    neighbours intact), with gapless trims, after `reset()`; two registry-built decoders share the batcher's launches.

The frozen runs (tests/golden/mpa12) are replayed on the GPU by the gpu-marked test at the end, which reads the fixtures only."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import mpa12_writer as W  # noqa: E402
from emu_lib import emu_ctx  # noqa: F401,E402

localref = pytest.mark.localref  # (every test but the gpu-marked replay at the end needs the reference tree)


@localref
def test_fixtures_regenerate_from_the_reference_tree():
    import make_mpa12_fixtures as M
    tables, streams = M.generate()
    assert M.compare(tables, dict(np.load(M.OUT / "tables.npz"))) == []
    assert M.compare(streams, dict(np.load(M.OUT / "streams.npz"))) == []


def damaged(layer, packet, how):
    b = bytearray(packet)
    if how == "short":
        return bytes(b[:len(b) // 3])  # the sample reads run out
    assert layer == 1
    b[4] |= 0xf0  # the first allocation nibble becomes 15
    return bytes(b)


@localref
@pytest.mark.parametrize("layer,how", [(1, "alloc15"), (1, "short"), (2, "short")])
def test_a_refused_packet_fails_alone_and_leaves_the_state(emu_ctx, layer, how):  # noqa: F811
    import make_mpa12_fixtures as M
    import rs_harness as H
    from symphonia_amd import Mpa12Decode
    rng = np.random.default_rng(70 + layer)
    h = W.Header(1, rate_idx=14, sr_idx=2, mode=W.STEREO) if layer == 1 else W.Header(2, rate_idx=14, sr_idx=2, mode=W.JOINT, mode_ext=1)
    make, frame, inputs = (W.random_layer1, W.layer1_frame, W.layer1_inputs) if layer == 1 else (W.random_layer2, W.layer2_frame, W.layer2_inputs)
    fields = [make(rng, h) for _ in range(3)]
    packets = [frame(h, *f) for f in fields]
    run = [packets[0], damaged(layer, packets[1], how), packets[1], damaged(layer, packets[2], how), packets[2]]
    it = M.interpreter(layer)
    # (the driver of the fixture generator checks the packet length as MpaDecoder does; a short packet goes to the layer as it is)
    it.load_source("""pub fn mpa12_packets_decode(layer: &mut dyn Layer, data: &[u8], buf: &mut AudioBuffer<f32>) -> Result<()> {
        let mut r = BufReader::new(data); let header = read_frame_header(&mut r)?; buf.clear(); layer.decode(&mut r, &header, buf) }""", "mpa12_packets_driver.rs")
    dec, buf = it.call("mpa12_fixture_new"), it.call("mpa12_fixture_buffer", H.u8_vec(packets[0]))
    ref_pcm, outcomes = [], []
    for p in run:
        r = it.call("mpa12_packets_decode", dec, H.u8_vec(p), buf)
        outcomes.append(r.variant)
        if r.variant == "Ok":
            ref_pcm.append(H.Harness.planes(buf))
    assert outcomes == ["Ok", "Err", "Ok", "Err", "Ok"]
    pairs = [inputs(h, *f) for f in fields]
    codes, rec = np.stack([c for c, _ in pairs], 1), np.stack([r for _, r in pairs], 1)
    got = Mpa12Decode(emu_ctx, layer).decode(codes, rec, np.zeros((2, 1024), np.float32), np.zeros(2, np.int32))
    assert np.array_equal(got[0].view(np.uint32), np.stack(ref_pcm, 1).view(np.uint32)) and not got[3].any()
    vvec, vfront = M.state_of(dec, 2)
    assert np.array_equal(got[1].view(np.uint32), vvec.view(np.uint32)) and np.array_equal(got[2], vfront)


SEAM_STREAMS = ("l1_stereo_crc", "l1_joint_b8", "l2_c_mono", "l2_b_joint_b8", "l2_m2_stereo")


@pytest.fixture(scope="module")
def patched_src():
    import rs_harness as H
    return H.patched_tree(("symphonia-bundle-mp3",)) / "symphonia-bundle-mp3" / "src"


@localref
@pytest.mark.parametrize("name", SEAM_STREAMS)
def test_the_patched_layers_with_and_without_a_backend(patched_src, name):
    import json
    import make_mpa12_fixtures as M
    import rs_harness as H
    s = np.load(M.OUT / "streams.npz")
    e = next(x for x in json.loads(bytes(s["manifest"]).decode())["entries"] if x["name"] == name)
    layer, nch, nf = e["layer"], e["channels"], 12 if e["layer"] == 1 else 36
    it = M.interpreter(layer, patched_src, ("backend.rs",))
    it.load_file(ROOT / "tests" / "rust" / "mpa12_stubs.rs")
    it.load_source("pub fn mpa12_seam_new() -> Layer%d { Layer%d::with_backend(mpa12_recording_backend()) }" % (layer, layer), "mpa12_seam_driver.rs")
    packets = s[name + "_packets"]
    # without a backend: every result is what it is today
    dec, buf = it.call("mpa12_fixture_new"), it.call("mpa12_fixture_buffer", H.u8_vec(packets[0]))
    for i, p in enumerate(packets):
        assert it.call("mpa12_fixture_decode", dec, H.u8_vec(p), buf).variant == "Ok"
        assert np.array_equal(H.Harness.planes(buf).view(np.uint32), s[name + "_pcm"][:, i]), (name, i)
    vvec, vfront = M.state_of(dec, nch)
    assert np.array_equal(vvec.view(np.uint32), s[name + "_vvec"]) and np.array_equal(vfront, s[name + "_vfront"])
    # with the recording backend: the frames are the writer's fields
    dec = it.call("mpa12_seam_new")
    for p in packets:
        assert it.call("mpa12_fixture_decode", dec, H.u8_vec(p), buf).variant == "Ok"
        assert int(buf.f["num_frames"].v) == 32 * nf
    backend = H.I.deref(dec.f["backend"].f["0"])
    assert backend.name == "RecordingSubband" and len(backend.f["frames"].a) == len(packets)
    for i, fr in enumerate(backend.f["frames"].a):
        fr = H.I.deref(fr)
        assert int(fr.f["layer"].v) == layer and int(fr.f["num_channels"].v) == nch
        codes = np.array([[x.v for x in row.a] for row in fr.f["codes"].a], np.uint16)
        rec = np.array([[x.v for x in row.a] for row in fr.f["rec"].a], np.uint8)
        assert np.array_equal(codes[:nch, :32 * nf].reshape(nch, 32, nf), s[name + "_codes"][:, i]), (name, i)
        assert np.array_equal(rec[:nch, :64 * layer], s[name + "_rec"][:, i]) and not rec[:, 64 * layer:].any() and not codes[:, 32 * nf:].any(), (name, i)
    vvec, vfront = M.state_of(dec, nch)
    assert not vvec.any() and not vfront.any()


@localref
def test_the_patched_decoder_with_a_sub_band_backend(patched_src):
    """`MpaDecoder::try_new_with_subband_backend` (built with the three layer features): packets of both layers cross the seam frame by
    frame, a damaged packet fails with the reference's error and records nothing, `reset()` keeps the backend and resets it, and a
    Layer III codec is refused.  (Both layers' files in one interpreter: their private `dequantize` functions share a name, which the
    path WITH a backend never calls.)"""
    import json
    import make_mpa12_fixtures as M
    import rs_harness as H
    I = H.I
    h = H.Harness(None, reference=True, sample="f32")
    it = h.it
    for f in H.MP3_FILES + ("backend.rs", "layer12.rs", "layer1/mod.rs", "layer2/mod.rs"):
        it.load_file(patched_src / f)
    it.load_file(ROOT / "tests" / "rust" / "mpa12_stubs.rs")
    it.load_source(H.cfg_features((patched_src / "decoder.rs").read_text(), {"mp1", "mp2", "mp3"}), "decoder.rs")
    assert not it.globals.get("__unparsed__"), it.globals.get("__unparsed__")
    s = np.load(M.OUT / "streams.npz")
    entries = {x["name"]: x for x in json.loads(bytes(s["manifest"]).decode())["entries"]}
    for name, codec in (("l1_stereo_crc", "CODEC_ID_MP1"), ("l2_c_mono", "CODEC_ID_MP2")):
        e = entries[name]
        layer, nch, nf = e["layer"], e["channels"], 12 if e["layer"] == 1 else 36
        r = it.call("MpaDecoder::try_new_with_subband_backend", h.params(codec, e["sample_rate"], nch), h.opts(), it.call("mpa12_recording_backend"))
        assert r.variant == "Ok", r
        dec = r.f["0"]
        packets = [bytes(p) for p in s[name + "_packets"]]
        run = [packets[0], packets[1][:len(packets[1]) // 2], packets[1]]
        results = [h.decode("MpaDecoder", dec, h.packet(p, 32 * nf * i)) for i, p in enumerate(run)]
        assert [x[0] for x in results] == ["ok", "err", "ok"] and results[1][1] == "DecodeError" and results[0][1].shape == (nch, 32 * nf)
        layer_state = I.deref(dec.f["state"].f["0"])
        backend = I.deref(layer_state.f["backend"].f["0"])
        assert len(backend.f["frames"].a) == 2 and int(backend.f["resets"].v) == 0
        for i, fr in enumerate(backend.f["frames"].a):
            codes = np.array([[x.v for x in row.a] for row in I.deref(fr).f["codes"].a], np.uint16)
            assert np.array_equal(codes[:nch, :32 * nf].reshape(nch, 32, nf), s[name + "_codes"][:, i]), (name, i)
        it.call_method("MpaDecoder", "reset", dec)
        backend = I.deref(I.deref(dec.f["state"].f["0"]).f["backend"].f["0"])
        assert backend.name == "RecordingSubband" and int(backend.f["resets"].v) == 1
    r = it.call("MpaDecoder::try_new_with_subband_backend", h.params("CODEC_ID_MP3", 44100, 2), h.opts(), it.call("mpa12_recording_backend"))
    assert r.variant == "Err" and r.f["0"].variant == "Unsupported", r


# ---- written packets three ways: the unpatched MpaDecoder, its patched twin without a backend, HipMpa12Decoder on the emulation library

CODEC = {1: "CODEC_ID_MP1", 2: "CODEC_ID_MP2"}


def decoder_harness(layer, src, dll=None):
    """the MP3 crate at `src` built with the ONE layer feature (the two layers' files share private function names), symphonia-core's own
    io / packet modules; with `dll`, the shim crate on top of it"""
    import rs_harness as H
    h = H.Harness(dll, reference=True, sample="f32")
    it = h.it
    it.load_file(ROOT / "tests" / "rust" / "mpa12_stubs.rs")
    for f in ("common.rs", "header.rs", "layer12.rs", "synthesis.rs") + (("backend.rs",) if (src / "backend.rs").exists() else ()) + ("layer%d/mod.rs" % layer,):
        it.load_file(src / f)
    it.load_source(H.cfg_features((src / "decoder.rs").read_text(), {"mp%d" % layer}), "decoder.rs")
    if dll is not None:
        it.load_file(ROOT / "tests" / "rust" / "registry_stubs.rs")
        h.load_shim("lib.rs", "ctx.rs", "decoder.rs", "lookahead.rs", "fallback.rs", "pcm.rs", "mpa12.rs", "mpa12/decoder.rs")
    assert not it.globals.get("__unparsed__"), it.globals.get("__unparsed__")
    return h


def mpa_decoder(h, layer, e, gapless=True):
    r = h.it.call("MpaDecoder::try_new", h.params(CODEC[layer], e["sample_rate"], e["channels"]), h.opts(gapless=gapless))
    assert r.variant == "Ok", r
    return r.f["0"]


def hip_decoder(h, layer, e, max_batch, gapless=True):
    r = h.it.call("HipMpa12Decoder::try_new", h.params(CODEC[layer], e["sample_rate"], e["channels"]), h.opts(gapless=gapless), H_usize(max_batch))
    assert r.variant == "Ok", r
    return r.f["0"]


def H_usize(v):
    import rs_harness as H
    return H.usize(v)


def trimmed(h, data, pts, start=0, end=0, owned=False, track=0):
    import rs_harness as H
    p = h.packet(data, pts, track=track, owned=owned)
    p.f["trim_start"] = H.I.Struct("Duration", {"0": H.I.Int(int(start), "u64")})
    p.f["trim_end"] = H.I.Struct("Duration", {"0": H.I.Int(int(end), "u64")})
    return p


def written_stream(layer, n, seed):
    """(header entry, [packet bytes]) of n frames of one stereo stream"""
    rng = np.random.default_rng(seed)
    h = W.Header(1, rate_idx=14, sr_idx=2, mode=W.JOINT, mode_ext=1) if layer == 1 else W.Header(2, rate_idx=14, sr_idx=2, mode=W.JOINT, mode_ext=2, crc=True)
    make, frame = (W.random_layer1, W.layer1_frame) if layer == 1 else (W.random_layer2, W.layer2_frame)
    return {"sample_rate": h.sample_rate, "channels": h.channels}, [frame(h, *make(rng, h)) for _ in range(n)]


def same(a, b):
    return a[0] == b[0] and (np.array_equal(np.asarray(a[1]).view(np.uint32), np.asarray(b[1]).view(np.uint32)) if a[0] == "ok" else a[1] == b[1])


@localref
@pytest.mark.parametrize("layer", [1, 2])
def test_three_decoders_agree_on_written_packets(patched_src, layer):
    """the reference's unpatched MpaDecoder, the patched one without a backend and HipMpa12Decoder (look-ahead batches of 3 behind a
    LookaheadReader, so the 7 packets cross two batch boundaries): bit for bit, with a damaged packet in mid-batch (the same error
    from all three, the neighbours intact), gapless trims on the first and the last packet, and again after reset()"""
    import rs_harness as H
    from emu_lib import emu_library
    I = H.I
    e, packets = written_stream(layer, 7, 300 + layer)
    frames = 384 if layer == 1 else 1152
    run = list(packets)
    run[4] = packets[4][:len(packets[4]) // 2]  # damaged: the packet is not the length its header states
    trims = {0: (100, 0), 6: (0, 57)}
    ref_h, twin_h = decoder_harness(layer, H.REF / "symphonia-bundle-mp3" / "src"), decoder_harness(layer, patched_src)
    hip_h = decoder_harness(layer, patched_src, emu_library().dll)
    hip_h.it.load_file(ROOT / "tests" / "rust" / "mocks.rs")
    ref, twin, hip = mpa_decoder(ref_h, layer, e), mpa_decoder(twin_h, layer, e), hip_decoder(hip_h, layer, e, 3)
    owned = I.Arr([trimmed(hip_h, p, frames * i, *trims.get(i, (0, 0)), owned=True, track=1) for i, p in enumerate(run)], True)
    reader = hip_h.it.call("LookaheadReader::new", hip_h.it.call("MockReader::new", owned), H.usize(8))

    def three(first, count):
        out = []
        for i in range(first, first + count):
            a = ref_h.decode("MpaDecoder", ref, trimmed(ref_h, run[i], frames * i, *trims.get(i, (0, 0))))
            b = twin_h.decode("MpaDecoder", twin, trimmed(twin_h, run[i], frames * i, *trims.get(i, (0, 0))))
            r = hip_h.it.call_method("LookaheadReader", "next_packet", reader)
            c = hip_h.decode("HipMpa12Decoder", hip, hip_h.it.call_method("Packet", "as_packet_ref", r.f["0"].f["0"]))
            assert same(a, b), ("patched twin", i, a[0], b[0])
            assert same(a, c), ("HipMpa12Decoder", i, a, c)
            out.append(a)
        return out

    n0 = hip_h.bridge.calls.count("symaccel_mpa12_decode")
    got = three(0, 7)
    assert [g[0] for g in got] == ["ok"] * 4 + ["err"] + ["ok"] * 2 and got[4][1] == "DecodeError"
    assert got[0][1].shape == (2, frames - 100) and got[6][1].shape == (2, frames - 57) and got[1][1].shape == (2, frames)
    # packets 0-2 | 3 (the look-ahead stops in front of the damaged packet) | 4 fails alone, nothing launched | 5, 6
    assert hip_h.bridge.calls.count("symaccel_mpa12_decode") - n0 == 3
    # a seek: every decoder is reset and packets 2.. are decoded again from a zeroed state
    hip_h.it.call_method("LookaheadReader", "seek", reader, I.Int(0, "i64"), H.usize(2))
    for h_, d_, name in ((ref_h, ref, "MpaDecoder"), (twin_h, twin, "MpaDecoder"), (hip_h, hip, "HipMpa12Decoder")):
        h_.it.call_method(name, "reset", d_)
    again = three(2, 2)
    assert again[0][0] == "ok" and not same(again[0], got[2])  # (the history is gone: not the PCM of the first pass)


@localref
def test_registry_built_decoders_share_launches(patched_src):
    """`mpa12::register` enters HipMpa12Decoder at Tier::Preferred for MP1 / MP2; two decoders the registry builds from (params, opts)
    alone find each other in the process-wide Pool: their batches go out in common launches, and every packet is the reference's PCM"""
    import rs_harness as H
    from emu_lib import emu_library
    I = H.I
    layer, n, depth = 2, 6, 3
    e, _ = written_stream(layer, 0, 0)
    streams = [written_stream(layer, n, 400 + k)[1] for k in range(2)]
    ref_h = decoder_harness(layer, H.REF / "symphonia-bundle-mp3" / "src")
    refs = [mpa_decoder(ref_h, layer, e) for _ in range(2)]
    h = decoder_harness(layer, patched_src, emu_library().dll)
    it = h.it
    it.load_file(ROOT / "tests" / "rust" / "mocks.rs")
    it.load_file(ROOT / "tests" / "rust" / "registry_generic.rs")
    reg = it.call("CodecRegistry::new")
    it.call("mpa12::register", reg)
    p = h.params(CODEC[layer], e["sample_rate"], e["channels"])
    decs = []
    for _ in range(2):
        r = it.call_method("CodecRegistry", "make_registered_audio_decoder", reg, p, h.opts())
        assert r.variant == "Ok", r
        dec = I.deref(r.f["0"])
        assert isinstance(dec, I.Struct) and dec.name == "HipMpa12Decoder", dec  # no fall-back taken
        decs.append(dec)
    readers = []
    for k, pk in enumerate(streams):
        owned = I.Arr([trimmed(h, data, 1152 * i, owned=True, track=1 + k) for i, data in enumerate(pk)], True)
        readers.append(it.call("LookaheadReader::new", it.call("MockReader::new", owned), H.usize(depth)))
    for i in range(n):
        for k in range(2):
            r = it.call_method("LookaheadReader", "next_packet", readers[k])
            got = h.decode("HipMpa12Decoder", decs[k], it.call_method("Packet", "as_packet_ref", r.f["0"].f["0"]))
            want = ref_h.decode("MpaDecoder", refs[k], trimmed(ref_h, streams[k][i], 1152 * i))
            assert same(want, got) and got[0] == "ok", (k, i)
    calls = h.bridge.calls
    assert calls.count("symaccel_batcher_create") == 1 and calls.count("symaccel_batcher_reserve") >= 2
    assert calls.count("symaccel_mpa12_decode") == 2  # each stream's cold start only: every later batch went through the batcher
    stats = H.pool_stats(h)
    assert stats["submissions"] >= 2 and stats["launches"] < stats["submissions"] and stats["failed_tickets"] == 0, stats
    # a codec this decoder does not take goes to the decoder below: with none registered, the reason comes back as Unsupported
    r = it.call("HipMpa12Decoder::try_registry_new", h.params("CODEC_ID_MP3", 44100, 2), h.opts())
    assert r.variant == "Err" and r.f["0"].variant == "Unsupported", r
    r = it.call("HipMpa12Decoder::try_registry_new", h.params(CODEC[layer], None, 2), h.opts())
    assert r.variant == "Err" and r.f["0"].variant == "Unsupported", r


# ---- GPU: the frozen runs of the interpreted reference, through the cross-stream batcher (reads tests/golden/mpa12 only)

@pytest.mark.gpu
def test_gpu_frozen_runs_replayed_through_the_batcher():
    import json
    import torch
    from symphonia_amd import BATCH_MPA12_DECODE, Batcher, Context
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    golden = ROOT / "tests" / "golden" / "mpa12" / "streams.npz"
    s = np.load(golden)
    with Context(0) as ctx:
        b = Batcher(ctx)
        subs = []
        for e in json.loads(bytes(s["manifest"]).decode())["entries"]:
            n, nch = e["name"], e["channels"]
            codes, rec = np.ascontiguousarray(s[n + "_codes"]), np.ascontiguousarray(s[n + "_rec"])
            vv, vf = np.zeros((nch, 1024), np.float32), np.zeros(nch, np.int32)
            pcm = np.full(codes.shape[:2] + (codes.shape[2] * codes.shape[3],), np.nan, np.float32)
            subs.append((b.submit(BATCH_MPA12_DECODE, e["layer"], [codes, rec], [vv, vf], pcm), n, pcm, vv, vf))
        for t, n, pcm, vv, vf in subs:
            b.collect(t)
            assert np.array_equal(pcm.view(np.uint32), s[n + "_pcm"]) and np.array_equal(vv.view(np.uint32), s[n + "_vvec"]), n
            assert np.array_equal(vf, s[n + "_vfront"]), n
        st = b.stats()
        assert st["launches"] < st["submissions"] == len(subs) and st["failed_tickets"] == 0, st
        b.close()
