"""FLAC streams with their TRUE MD5 in STREAMINFO, decoded with `verify: true` two ways (the harness of tests/test_flac_packets.py):

  frames written by tests/flac_writer.py; STREAMINFO carries hashlib's MD5 of the encoder's input as validate.rs hashes it
     |
     +--> the REFERENCE: symphonia-bundle-flac's FlacDecoder with its own Validator (validate.rs) over symphonia-core's Md5
     |    (checksum/md5.rs), EXECUTED from /root/reference by tools/rsinterp  ..............  finalize() == Some(true), PCM_ref
     |
     +--> HipFlacDecoder built by the registry (`make_audio_decoder(params, opts)` with verify: true -> try_registry_new -> the
          process-wide Pool): SeamFrontEnd reads the expected digest out of STREAMINFO, the look-ahead batches take the verify form
          of SYMACCEL_BATCH_FLAC_RESTORE, the first batch is hashed by symaccel_flac_md5  ...  finalize() == Some(true), == PCM_ref

A stream with a packet damaged in mid-batch: both decoders fail that packet, agree on the PCM of every other one and on Some(false).
Needs /root/reference (`localref`); the scripted twin with its `-m gpu` form is tests/test_rust_flac_verify.py."""
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import flac_writer as W  # noqa: E402
from rs_harness import REF, Harness, patched_tree, pool_stats, registry_round_trip, sized, usize  # noqa: E402
from rsinterp import interp as I  # noqa: E402
from test_flac_md5 import pack  # noqa: E402
from test_flac_packets import left_justified  # noqa: E402

pytestmark = pytest.mark.localref


def streaminfo(blocksize, rate, nch, bps, md5):
    bw = W.BitWriter()
    for v, n in ((blocksize, 16), (blocksize, 16), (0, 24), (0, 24), (rate, 20), (nch - 1, 3), (bps - 1, 5), (0, 36)):
        bw.put(v, n)
    for b in md5:
        bw.put(b, 8)
    return bw.bytes()


def true_md5(pcm, nch, bps):
    """validate.rs over the encoder's input: every frame's samples, ceil(bps / 8) little-endian bytes each, interleaved"""
    return hashlib.md5(b"".join(pack(np.asarray(p, np.int64), nch, [p.shape[1]], [0], (bps + 7) // 8) for p in pcm)).digest()


@pytest.fixture(scope="module")
def trees():
    return REF / "symphonia-bundle-flac" / "src", patched_tree(("symphonia-bundle-flac",)) / "symphonia-bundle-flac" / "src"


def verified_params(h, blocksize, nch, bps, md5):
    p = h.params("CODEC_ID_FLAC", extra=streaminfo(blocksize, 44100, nch, bps, md5))
    p.f["verification_check"] = I.NONE  # (the field the stand-in record lacks: the decoder fills it from STREAMINFO)
    return p


def reference_decoder(tree, blocksize, nch, bps, md5):
    """the reference's FlacDecoder with verify: true, its Validator and symphonia-core's Md5 loaded over the stand-ins"""
    h = Harness(None, reference=True, flac_tree=tree)
    h.it.load_file(ROOT / "tests" / "rust" / "flac_verify_core_stubs.rs")
    h.it.load_file(REF / "symphonia-core" / "src" / "checksum" / "md5.rs")
    h.it.load_file(REF / "symphonia-bundle-flac" / "src" / "validate.rs")
    r = h.it.call("FlacDecoder::try_new", verified_params(h, blocksize, nch, bps, md5), h.opts(verify=True))
    assert r.variant == "Ok", r
    return h, r.f["0"]


def registry_decoder(tree, blocksize, nch, bps, md5):
    from emu_lib import emu_library
    h = Harness(emu_library().dll, reference=True, flac_tree=tree)
    for f in ("registry_stubs.rs", "mocks.rs", "flac_verify_core_stubs.rs"):
        h.it.load_file(ROOT / "tests" / "rust" / f)
    h.load_shim("lib.rs", "ctx.rs", "decoder.rs", "lookahead.rs", "fallback.rs", "flac.rs", "frontends.rs")
    # (registry_round_trip asserts that what the registry built IS a HipFlacDecoder: the fall-back factory was not reached)
    dec = registry_round_trip(h, "HipFlacDecoder", [verified_params(h, blocksize, nch, bps, md5)], opts=h.opts(verify=True))[0]
    return h, dec


def verdict(h, type_name, dec):
    v = h.it.call_method(type_name, "finalize", dec).f["verify_ok"]
    return None if v.variant == "None" else bool(v.f["0"])


def decode_both(trees, frames, pcm, nch, bps, blocksize, md5, depth):
    ref, ref_dec = reference_decoder(trees[0], blocksize, nch, bps, md5)
    h, dec = registry_decoder(trees[1], blocksize, nch, bps, md5)
    packets = I.Arr([h.packet(fr, i * blocksize, track=1, owned=True) for i, fr in enumerate(frames)], True)
    reader = h.it.call("LookaheadReader::new", h.it.call("MockReader::new", packets), usize(depth))
    outcomes = []
    for i, fr in enumerate(frames):
        st_r, want = ref.decode("FlacDecoder", ref_dec, ref.packet(fr, i * blocksize))
        r = h.it.call_method("LookaheadReader", "next_packet", reader)
        st, got = h.decode("HipFlacDecoder", dec, h.it.call_method("Packet", "as_packet_ref", r.f["0"].f["0"]))
        assert st == st_r, (i, st, st_r, got, want)
        if st == "ok":
            assert np.array_equal(got, want), i
            if pcm is not None:
                assert np.array_equal(want, left_justified(pcm[i], bps)), i
        outcomes.append(st)
    return ref, ref_dec, h, dec, outcomes


STREAMS = [(31, 13, 2, 16, 192), (32, 9, 2, 24, 100), (33, 9, 1, 16, 576)]


@pytest.mark.parametrize("seed,n_frames,nch,bps,blocksize", sized(STREAMS, STREAMS[:2]))
def test_a_stream_with_its_true_md5_verifies_in_both_decoders(trees, seed, n_frames, nch, bps, blocksize):
    frames, pcm = W.random_stream(seed, n_frames, nch, bps, blocksize)
    md5 = true_md5(pcm, nch, bps)
    ref, ref_dec, h, dec, outcomes = decode_both(trees, frames, pcm, nch, bps, blocksize, md5, depth=4)
    assert outcomes == ["ok"] * n_frames
    assert verdict(ref, "FlacDecoder", ref_dec) is True, "the reference's own validator must accept the stream"
    assert verdict(h, "HipFlacDecoder", dec) is True
    calls = h.bridge.calls
    # the cold start is the decoder's own batch (hashed by symaccel_flac_md5), every later batch took the batcher's verify form
    assert calls.count("symaccel_flac_md5") == 1 and calls.count("symaccel_batcher_reserve") >= 2, [c for c in calls if "md5" in c or "batcher" in c]
    reserved = [args["param"] for name, args in h.bridge.scalars if name == "symaccel_batcher_reserve"]
    assert reserved and all(prm == 0x200 | (nch - 1) << 12 for prm in reserved), [hex(prm) for prm in reserved]  # the verify form itself
    stats = pool_stats(h)
    assert stats["submissions"] >= 2 and stats["failed_tickets"] == 0, stats


def test_a_damaged_packet_in_mid_batch_fails_the_digest_in_both_decoders(trees):
    nch, bps, blocksize = 2, 16, 192
    frames, pcm = W.random_stream(35, 11, nch, bps, blocksize)
    md5 = true_md5(pcm, nch, bps)
    stream = list(frames)
    broken = bytearray(stream[6])
    broken[3] ^= 0x10  # a header bit: CRC-8 mismatch -- the packet contributes no frame (decoder.rs returns before line 232)
    stream[6] = bytes(broken)
    ref, ref_dec, h, dec, outcomes = decode_both(trees, stream, None, nch, bps, blocksize, md5, depth=4)
    assert outcomes.count("err") == 1 and outcomes[6] == "err"
    assert verdict(ref, "FlacDecoder", ref_dec) is False
    assert verdict(h, "HipFlacDecoder", dec) is False
