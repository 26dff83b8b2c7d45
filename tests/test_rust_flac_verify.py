"""`HipFlacDecoder` with `AudioDecoderOptions::verify` -- bindings/rust/symphonia-accel-hip/src/{flac,decoder,lookahead}.rs EXECUTED under
the repository's Rust interpreter, the harness of tests/test_rust_adapters.py, with a scripted front end that supplies `expected_md5`
(tests/rust/flac_verify_mocks.rs).  A pooled decoder's look-ahead batches take the verify form of SYMACCEL_BATCH_FLAC_RESTORE (param
0x200 | (nch - 1) << 12); its first batch, transformed by the decoder itself, is hashed by symaccel_flac_md5.  The digest `finalize()`
compares is that of the packets HANDED OUT: across batch boundaries, after reset() (the reference keeps its validator across reset,
decoder.rs:254-256) and around packets the caller skipped (the one-packet replay hashes nothing).  The expected digests are hashlib's
over the bytes validate.rs would hash of the encoder's input PCM.  CPU emulation here, the hipcc-built library in the gpu twins."""
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

from rs_harness import usize  # noqa: E402
from rsinterp import interp as I  # noqa: E402
from test_flac_md5 import pack  # noqa: E402
from test_rust_adapters import LIBS, flac_script, harness, key, wrap32  # noqa: E402

BPS, BLOCKSIZE, NFR, NCH = 16, 96, 13, 2


def hashed(pcm):
    """validate.rs: the bytes each frame feeds the MD5 -- the decoded samples, (bps + 7) / 8 little-endian bytes each, interleaved"""
    return [pack(np.asarray(p, np.int64), NCH, [p.shape[1]], [0], (BPS + 7) // 8) for p in pcm]


def md5_of(chunks):
    return hashlib.md5(b"".join(chunks)).digest()


def some_digest(d):
    return I.some(I.Arr([I.Int(b, "u8") for b in d], False))


def build(make_dll, expected, seed=900, flip=None, pooled=True, verify=True):
    """a verifying HipFlacDecoder over the scripted stream behind a LookaheadReader (look-ahead batches of 4); `expected`: a digest, or
    a function of the frames' hashed bytes, or None (no MD5 in STREAMINFO)"""
    h = harness(make_dll, "flac.rs")
    h.it.load_file(ROOT / "tests" / "rust" / "mocks.rs")
    h.it.load_file(ROOT / "tests" / "rust" / "flac_verify_mocks.rs")
    script, pcm = flac_script(np.random.default_rng(seed), BPS, BLOCKSIZE, NFR)
    chunks = hashed(pcm)
    if flip is not None:
        w = script[flip].f["words"].a
        w[7] = I.Int(w[7].v ^ 1, "i32")
    digest = expected(chunks) if callable(expected) else expected
    params = h.params("CODEC_ID_FLAC", 44100, NCH, bps=BPS)
    front = I.Struct("VerifiedFlacFront", {"params": params, "nch": usize(NCH), "max_bs": usize(BLOCKSIZE), "script": I.Arr(script, True),
                                            "parses": usize(0), "md5": some_digest(digest) if digest is not None else I.NONE})
    r = h.it.call("HipFlacDecoder::try_new_pooled" if pooled else "HipFlacDecoder::try_new", params, h.opts(verify=verify), front, usize(4))
    if r.variant != "Ok":
        return h, r, None, pcm, chunks
    packets = I.Arr([h.packet(key(t), BLOCKSIZE * t, track=7, owned=True) for t in range(NFR)], True)
    reader = h.it.call("LookaheadReader::new", h.it.call("MockReader::new", packets), usize(12))
    return h, r.f["0"], reader, pcm, chunks


def step(h, dec, reader, pcm, t, compare=True):
    """the reader's next packet (it must be packet t) through decode_ref"""
    r = h.it.call_method("LookaheadReader", "next_packet", reader)
    st, got = h.decode("HipFlacDecoder", dec, h.it.call_method("Packet", "as_packet_ref", r.f["0"].f["0"]))
    assert st == "ok", (t, got)
    if compare:
        assert np.array_equal(got, wrap32(pcm[t].astype(np.int64) << (32 - BPS))), t


def skip(h, reader):
    h.it.call_method("LookaheadReader", "next_packet", reader)


def verdict(h, dec):
    v = h.it.call_method("HipFlacDecoder", "finalize", dec).f["verify_ok"]
    return None if v.variant == "None" else bool(v.f["0"])


@pytest.mark.parametrize("make_dll", LIBS)
def test_a_verified_stream_across_batch_boundaries(make_dll):
    h, dec, reader, pcm, chunks = build(make_dll, md5_of)
    assert verdict(h, dec) is False  # (nothing handed out yet: the digest of nothing is not the stream's)
    for t in range(NFR):
        step(h, dec, reader, pcm, t)
    assert verdict(h, dec) is True
    calls = h.bridge.calls
    # the first batch is the decoder's own (restore + symaccel_flac_md5), the others went through the batcher's verify form
    assert calls.count("symaccel_flac_md5") == 1 and calls.count("symaccel_batcher_reserve") == 3, [c for c in calls if "batcher" in c or "md5" in c]
    assert "symaccel_flac_restore" in calls
    reserved = [args["param"] for name, args in h.bridge.scalars if name == "symaccel_batcher_reserve"]
    assert reserved == [0x200 | (NCH - 1) << 12] * 3, [hex(prm) for prm in reserved]


@pytest.mark.parametrize("make_dll", LIBS)
def test_a_flipped_residual_bit_fails_the_digest(make_dll):
    h, dec, reader, pcm, chunks = build(make_dll, md5_of, flip=5)
    for t in range(NFR):
        step(h, dec, reader, pcm, t, compare=t != 5)
    assert verdict(h, dec) is False


@pytest.mark.parametrize("make_dll", LIBS)
def test_no_digest_in_streaminfo_and_verify_off_give_no_verdict(make_dll):
    h, dec, reader, pcm, chunks = build(make_dll, None)
    for t in range(NFR):
        step(h, dec, reader, pcm, t)
    assert verdict(h, dec) is None
    h, dec, reader, pcm, chunks = build(make_dll, md5_of, verify=False)
    for t in range(5):
        step(h, dec, reader, pcm, t)
    assert verdict(h, dec) is None and "symaccel_flac_md5" not in h.bridge.calls


@pytest.mark.parametrize("make_dll", LIBS)
def test_without_the_batcher_verification_goes_to_the_decoder_below(make_dll):
    h, r, _, _, _ = build(make_dll, md5_of, pooled=False)
    assert r.variant == "Err" and r.f["0"].variant == "Unsupported"


@pytest.mark.parametrize("make_dll", LIBS)
def test_finalize_after_six_packets_is_the_digest_of_six_frames(make_dll):
    """the checkpoint rule: two batches were computed (and a third submitted), six packets were handed out"""
    h, dec, reader, pcm, chunks = build(make_dll, lambda c: md5_of(c[:6]))
    for t in range(6):
        step(h, dec, reader, pcm, t)
    assert verdict(h, dec) is True
    step(h, dec, reader, pcm, 6)
    assert verdict(h, dec) is False


@pytest.mark.parametrize("make_dll", LIBS)
def test_reset_keeps_the_hash_going(make_dll):
    h, dec, reader, pcm, chunks = build(make_dll, md5_of)
    for t in range(6):
        step(h, dec, reader, pcm, t)
    h.it.call_method("HipFlacDecoder", "reset", dec)
    for t in range(6, NFR):
        step(h, dec, reader, pcm, t)
    assert verdict(h, dec) is True


@pytest.mark.parametrize("make_dll", LIBS)
def test_skipped_packets_are_not_hashed_and_the_replay_hashes_nothing(make_dll):
    h, dec, reader, pcm, chunks = build(make_dll, lambda c: md5_of(c[:6] + c[8:]))
    for t in range(6):
        step(h, dec, reader, pcm, t)
    skip(h, reader)
    skip(h, reader)
    n_md5 = h.bridge.calls.count("symaccel_flac_md5")
    step(h, dec, reader, pcm, 8)
    # the replay of packet 5 restored it again and hashed nothing; the batch that starts at packet 8 is the decoder's own and is hashed
    assert h.bridge.calls.count("symaccel_flac_md5") == n_md5 + 1
    for t in range(9, NFR):
        step(h, dec, reader, pcm, t)
    assert verdict(h, dec) is True
