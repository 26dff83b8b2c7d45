"""PCM and G.711 on the device: symaccel_pcm_decode(_device) against symphonia-codec-pcm.

Expected samples come from two places that must agree:
  * tests/golden/pcm_decode.npz -- the reference's own PcmDecoder::try_new + decode_ref executed under tools/rsinterp on packet sequences
    of all twenty codecs (a long packet, a short one after it, an empty one, one frame, a trailing partial frame, one above
    max_frames_per_packet: frame counts, buffer variants and planes), the refusals of try_new, and the reference's reads, shifts,
    FromSample conversions and log expansions sample by sample (tools/make_pcm_decode_fixtures.py says exactly what runs and which
    stand-ins it uses; the localref case regenerates and compares);
  * tests/pcm_decode_ref.py -- a numpy restatement written from the reference's text, pinned to the fixture bit for bit and, exhaustively,
    to scalar forms: all 256 codes of the five 1-byte codecs at every legal shift, all 65 536 codes of the four 16-bit codecs at shift 0
    and 15.
The kernel is checked on the fixture's bytes and on arbitrary bytes against the restatement for every shape at which it takes another
path.  Every comparison is on bytes, no tolerance; guard bytes surround every output, and the input buffer ends with the last packet's
last byte.  CPU emulation here, gpu-marked twins on the MI355X."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from emu_lib import emu_ctx, emu_library  # noqa: F401
from symphonia_amd import Context, SymaccelError, pcm_coded_bytes, pcm_decode, pcm_decode_device, pcm_native_bytes, PCM_CODECS
from symphonia_amd import _ffi
from test_pcm_convert import FMT, EmuDev, GpuDev

import pcm_decode_ref as R

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
GOLDEN = ROOT / "tests" / "golden" / "pcm_decode.npz"
GUARD = 0xA5
# one codec per kernel source family and byte order: what the kernel instantiates and branches on
FAMILY_CODECS = ("u8", "s8", "s16le", "u16be", "s24le", "u24be", "s32be", "u32le", "f32le", "f32be", "f64le", "f64be", "alaw", "mulaw")


@pytest.fixture(scope="module")
def emu_dev(emu_ctx):  # noqa: F811
    return EmuDev(emu_ctx)


@pytest.fixture(scope="module")
def gpu_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on an MI355X (there is no CPU path)")
    dev = GpuDev(Context(0))
    yield dev
    dev.ctx.close()


def fixture():
    z = np.load(GOLDEN)
    return z, json.loads(bytes(z["manifest"]).decode())


def top_shift(codec):
    return max(R.legal_shifts(codec))


def run_device(dev, packets, codec, channels, frames, shift=0, fmt=0, pitch_pad=0, src_offset=0, dst_offset=0):
    """symaccel_pcm_decode_device on packets laid out at their bytes + pitch_pad, the first one src_offset bytes past an aligned address;
    -> uint8[n, bytes of a packet's output]; checks that nothing outside the output was written"""
    n, cb = packets.shape[0], R.coded_bytes(codec)
    nb = frames * channels * cb
    pitch = nb + pitch_pad
    rows = np.full((n, pitch), 0x5A, np.uint8)
    rows[:, :nb] = packets[:, :nb]
    src = np.concatenate([np.full(src_offset, 0x5A, np.uint8), rows.ravel()[:max(n - 1, 0) * pitch + nb]])  # (the last packet ends the buffer: nothing behind it may be read)
    ob = channels * frames * (R.native_bytes(codec) if fmt == 0 else R.DEST_BYTES[fmt])
    d_src, d_dst = dev.put(np.concatenate([src, np.zeros(0, np.uint8)]) if src.size else np.zeros(1, np.uint8)), dev.zeros(dst_offset + n * ob + 64, GUARD)
    pcm_decode_device(dev.ctx, dev.addr(d_src) + src_offset, pitch, n, codec, channels, shift, frames, dev.addr(d_dst) + dst_offset, 0 if fmt == 0 else FMT[fmt])
    out = dev.get(d_dst)
    assert np.all(out[:dst_offset] == GUARD) and np.all(out[dst_offset + n * ob:] == GUARD), "bytes outside the PCM were written"
    return out[dst_offset:dst_offset + n * ob].reshape(n, ob)


def native_bytes_of(planes):
    return np.ascontiguousarray(planes).view(np.uint8).reshape(planes.shape[0], -1)


# ---- the two expectations agree ----------------------------------------------------------------------------------------------------------

def test_restatement_equals_the_reference_fixture():
    z, m = fixture()
    assert m["overflows"] == 0
    seen = set()
    for e in m["entries"]:
        if "packets" in e:
            continue
        if "codec" in e:
            got = R.decode_samples(z[e["name"] + "_bytes"][:e["samples"] * R.coded_bytes(e["codec"])], e["codec"], e["shift"])
            want = z[e["name"] + "_native"]
            assert got.dtype == want.dtype and np.array_equal(got, want), e["name"]
            seen.add(e["codec"])
        else:
            src, dst = e["name"].split("_to_")
            x = z["in_" + src]
            native = x.view(np.float64) if src == "f64" else x.astype(R.NATIVE_DTYPE[src])
            assert np.array_equal(R.convert(src, dst, native), z[e["name"]]), e["name"]
    assert seen == set(R.NAMES) - {"f32le", "f32be", "f64le", "f64be"}  # (sample by sample; the float codecs are in the packet entries)
    assert {e["name"] for e in m["entries"] if "cases" in e} == {"%s_to_%s" % (s, d) for s in set(R.FAMILIES) - {"s32", "f32"} for d in R.DESTS}


def packet_entries():
    """(entry, packet index, bytes, frames, planes as the native type) of the reference decoder's recorded packets"""
    z, m = fixture()
    for e in m["entries"]:
        if "packets" in e:
            fam = R.CODECS[e["codec"]][3]
            for j, pk in enumerate(e["packets"]):
                planes = z["%s_p%d_planes" % (e["name"], j)]
                yield e, j, z["%s_p%d_bytes" % (e["name"], j)], pk, planes.view(R.NATIVE_DTYPE[fam]) if fam in ("f32", "f64") else planes


def test_restatement_equals_the_reference_decoder_on_packets():
    """frame count (a trailing partial frame dropped, an empty packet, a short packet after a long one, packets below and above
    max_frames_per_packet), buffer variant, de-interleave and sample values of PcmDecoder::decode_ref, all twenty codecs"""
    seen, lens = set(), set()
    for e, j, data, pk, planes in packet_entries():
        codec, ch = e["codec"], e["channels"]
        frames = R.frames_of(len(data), codec, ch)
        assert frames == pk["frames"] == planes.shape[1] and planes.shape[0] == ch and len(data) == pk["len"], (e["name"], j)
        assert pk["variant"].lower() == R.CODECS[codec][3], (e["name"], pk["variant"])
        got = R.decode(data[None, :], codec, ch, frames, e["shift"])[0]
        assert got.dtype == planes.dtype and np.array_equal(got.view(np.uint8), np.ascontiguousarray(planes).view(np.uint8)), (e["name"], j)
        seen.add((codec, e["shift"] != 0))
        lens.add((pk["frames"] == 0, len(data) % (R.coded_bytes(codec) * ch) != 0, pk["frames"] > e["max_frames_per_packet"]))
    assert {c for c, _ in seen} == set(R.NAMES) and {c for c, s in seen if s} == {c for c in R.NAMES if R.CODECS[c][1] in "su"}
    assert {(True, False, False), (True, True, False), (False, True, False), (False, False, True), (False, False, False)} <= lens


def test_try_new_refusals_are_recorded_with_the_reference_variants():
    _, m = fixture()
    r = {(x["codec"], x["sample_rate"], x["channels"], x["bits_per_sample"], x["bits_per_coded_sample"]): (x["error"], x["message"]) for x in m["try_new_refusals"]}
    assert r[("CODEC_ID_FLAC", 8000, 1, None, None)] == ("Unsupported", "pcm: invalid codec")
    assert r[("CODEC_ID_PCM_S16LE", None, 1, None, None)][0] == "Unsupported" and r[("CODEC_ID_PCM_S16LE", 8000, None, None, None)][0] == "Unsupported"
    assert all(v[0] == "DecodeError" for k, v in r.items() if k[3] is not None or k[4] is not None) and len(r) == 13


def test_i32_and_f32_sources_equal_the_existing_restatement():
    """the two source types the library already converted: tests/test_pcm_convert.py pins those to conv.rs"""
    from test_pcm_convert import restate, sweep_inputs
    for src in ("s32", "f32"):
        x = sweep_inputs(src)
        for dst in R.DESTS:
            assert np.array_equal(R.convert(src, dst, x), restate(src, dst, x)), (src, dst)


def test_one_byte_codecs_exhaustively():
    codes = np.arange(256, dtype=np.uint8)
    for codec in ("s8", "u8"):
        for shift in R.legal_shifts(codec):
            want = [R.int_scalar(int(c) - 256 if codec == "s8" and c > 127 else int(c), 8, codec == "s8", shift) for c in codes]
            assert R.decode_samples(codes, codec, shift).tolist() == want, (codec, shift)
    assert R.decode_samples(codes, "alaw").tolist() == [R.alaw_scalar(int(c)) for c in codes]
    assert R.decode_samples(codes, "mulaw").tolist() == [R.mulaw_scalar(int(c)) for c in codes]
    assert list(R.legal_shifts("alaw")) == [0] and list(R.legal_shifts("s8")) == list(range(8))
    # G.711's own landmarks: the largest and smallest magnitudes of the two laws
    assert R.alaw_scalar(0xAA) == 32256 and R.alaw_scalar(0x2A) == -32256 and R.alaw_scalar(0xD5) == 8 and R.alaw_scalar(0x55) == -8
    assert R.mulaw_scalar(0x80) == 32124 and R.mulaw_scalar(0x00) == -32124 and R.mulaw_scalar(0xFF) == 0 and R.mulaw_scalar(0x7F) == 0


def test_sixteen_bit_codecs_exhaustively():
    v = np.arange(65536, dtype=np.int64)
    le = np.stack([v & 0xff, v >> 8], axis=1).astype(np.uint8)
    for codec in ("s16le", "s16be", "u16le", "u16be"):
        signed, be = codec[0] == "s", codec.endswith("be")
        data = le[:, ::-1] if be else le
        for shift in (0, 15):
            x = (v << shift) & 0xffff
            want = np.where(x >> 15, x - 65536, x) if signed else x
            got = R.decode_samples(np.ascontiguousarray(data), codec, shift)
            assert np.array_equal(got.astype(np.int64), want), (codec, shift)


@pytest.mark.localref
def test_fixture_regenerates_from_the_reference_tree():
    import make_pcm_decode_fixtures as M
    assert M.compare(M.generate(), dict(np.load(GOLDEN))) == []


def test_byte_tables_and_constants():
    lib = emu_library()
    assert [PCM_CODECS[n] for n in R.NAMES] == list(range(1, 21))
    for name in R.NAMES:
        assert pcm_coded_bytes(name, lib) == R.coded_bytes(name) and pcm_native_bytes(name, lib) == R.native_bytes(name), name
    assert sorted({pcm_coded_bytes(n, lib) for n in R.NAMES}) == [1, 2, 3, 4, 8] and sorted({pcm_native_bytes(n, lib) for n in R.NAMES}) == [1, 2, 4, 8]
    for bad in (0, 21, -1, 255):
        assert pcm_coded_bytes(bad, lib) == 0 and pcm_native_bytes(bad, lib) == 0
    assert lib.dll.symaccel_abi_version() == 8 and lib.dll.symaccel_sample_bytes(10) == 0


# ---- the kernel --------------------------------------------------------------------------------------------------------------------------

def check_fixture(dev):
    """the fixture's bytes as one mono packet each (whole samples only: the fixture's multi-byte inputs end in a partial sample, which
    floor(len / coded bytes) drops, lib.rs:320)"""
    for e, j, data, pk, planes in packet_entries():  # the reference decoder's packets: multi-channel, every length class, a packet alone
        if pk["frames"]:
            got = run_device(dev, data[None, :], e["codec"], e["channels"], pk["frames"], shift=e["shift"], src_offset=1 + j)
            assert np.array_equal(got.ravel(), np.ascontiguousarray(planes).view(np.uint8).ravel()), (e["name"], j)
    z, m = fixture()
    for e in m["entries"]:
        if "codec" not in e or "packets" in e:
            continue
        data, want = z[e["name"] + "_bytes"], z[e["name"] + "_native"]
        frames = R.frames_of(len(data), e["codec"], 1)
        assert frames == len(want) == e["samples"]
        got = run_device(dev, data[None, :], e["codec"], 1, frames, shift=e["shift"], src_offset=3)
        assert np.array_equal(got.ravel(), want.view(np.uint8)), e["name"]


def check_all_codecs(dev):
    """all 20 codecs, shift 0 and the largest legal one, 3 channels, two tiles and a bit, three packets at an odd base and a padded pitch"""
    rng = np.random.default_rng(7)
    for codec in R.NAMES:
        cb, nb = R.coded_bytes(codec), R.native_bytes(codec)
        frames = R.tile_frames(3, cb, nb) * 2 + 5
        b = rng.integers(0, 256, (3, frames * 3 * cb), dtype=np.uint8)
        for shift in sorted({0, top_shift(codec)}):
            got = run_device(dev, b, codec, 3, frames, shift=shift, pitch_pad=7, src_offset=5, dst_offset=nb)
            assert np.array_equal(got, native_bytes_of(R.decode(b, codec, 3, frames, shift))), (codec, shift)


def check_tile_edges(dev, codec):
    """frames 0, 1, a tile minus 1, a tile, a tile plus 1, several tiles; channels 1, 2, 3, 8 (3-byte samples in 3 channels: a 9-byte frame)"""
    rng = np.random.default_rng(11)
    cb, nb = R.coded_bytes(codec), R.native_bytes(codec)
    for k, ch in enumerate((1, 2, 3, 8)):
        t = R.tile_frames(ch, cb, nb)
        assert t >= 16 and t % 16 == 0
        for frames in (0, 1, t - 1, t, t + 1, 3 * t + 2):
            b = rng.integers(0, 256, (2, max(frames * ch * cb, 1)), dtype=np.uint8)
            shift = (0, top_shift(codec))[k & 1]
            got = run_device(dev, b, codec, ch, frames, shift=shift, pitch_pad=(0, 3)[k & 1], src_offset=(0, 9, 1, 15)[k], dst_offset=nb * (k & 1))
            assert np.array_equal(got, native_bytes_of(R.decode(b, codec, ch, frames, shift))), (codec, ch, frames)


def check_alignments(dev):
    """source base offsets 0..15 with a padded pitch; output offsets of every legal alignment inside a 16-byte unit"""
    rng = np.random.default_rng(13)
    for codec, ch in (("s24be", 3), ("s16le", 2), ("mulaw", 1), ("f64be", 2)):
        cb, nb = R.coded_bytes(codec), R.native_bytes(codec)
        frames = R.tile_frames(ch, cb, nb) + 3
        b = rng.integers(0, 256, (3, frames * ch * cb), dtype=np.uint8)
        want = R.decode(b, codec, ch, frames)
        for s_off in range(16):
            got = run_device(dev, b, codec, ch, frames, pitch_pad=1 + s_off % 3, src_offset=s_off, dst_offset=(s_off * nb) % 16)
            assert np.array_equal(got, native_bytes_of(want)), (codec, s_off)
        fam = R.CODECS[codec][3]
        for fmt, offs in (("s16", range(0, 16, 2)), ("u24", range(16)), ("f32", range(0, 16, 4)), ("u8", range(16))):
            for d_off in offs:
                got = run_device(dev, b, codec, ch, frames, fmt=fmt, src_offset=d_off, dst_offset=d_off)
                assert np.array_equal(got, R.interleave(want, fam, fmt)), (codec, fmt, d_off)


def check_packet_counts(dev, many):
    """one packet; a count that does not fill the grid's first wave; more tiles than the grid holds (a workgroup walks several)"""
    rng = np.random.default_rng(17)
    for n, frames in ((1, 50), (3, 50), (many, 9)):
        b = rng.integers(0, 256, (n, frames * 2 * 2), dtype=np.uint8)
        got = run_device(dev, b, "s16be", 2, frames, src_offset=n % 16, pitch_pad=1)
        assert np.array_equal(got, native_bytes_of(R.decode(b, "s16be", 2, frames))), n
    cb, ch = 3, 2
    frames = R.tile_frames(ch, cb, 4) * 5 + 1  # one packet of more tiles than fit beside `many` packets
    b = rng.integers(0, 256, (many // 8, frames * ch * cb), dtype=np.uint8)
    got = run_device(dev, b, "u24le", ch, frames, fmt="s16")
    assert np.array_equal(got, R.interleave(R.decode(b, "u24le", ch, frames), "u24", "s16"))


FLOAT_TABLE_32 = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x00800000, 0x7f7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000,
                           0x7f800001, 0xff800001, 0x7fa55aa5, 0xffffffff, 0x3f800000, 0xbf800000], np.uint32)
FLOAT_TABLE_64 = np.array([0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x800fffffffffffff, 0x0010000000000000, 0x7fefffffffffffff,
                           0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff0000000000001,
                           0x7ff5a5a5a5a5a5a5, 0xffffffffffffffff, 0x3ff0000000000000, 0xbff0000000000000], np.uint64)


# ... and, for f64 -> f32 (`s as f32`): values in and around the f32 denormal range, halfway cases there, and both sides of the f32 overflow
F64_FOR_FORMATS = np.concatenate([FLOAT_TABLE_64, np.array([1e-40, -1e-40, 2.0 ** -126, 2.0 ** -127, 2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149,
                                                            -(2.0 ** -150), 3.4028234663852886e38, 3.4028235677973366e38, -3.4028235677973366e38, 3.5e38, 1e-46],
                                                           np.float64).view(np.uint64)])


def check_float_bits(dev):
    """NaN payloads, the infinities, denormals and -0.0 pass bit for bit, in both byte orders"""
    for codec, table in (("f32le", FLOAT_TABLE_32), ("f32be", FLOAT_TABLE_32), ("f64le", FLOAT_TABLE_64), ("f64be", FLOAT_TABLE_64)):
        le = table.view(np.uint8).reshape(len(table), -1)  # one frame of 1 channel per row; 2 channels x 8 frames below
        coded = (le[:, ::-1] if codec.endswith("be") else le).reshape(1, -1)
        got = run_device(dev, np.ascontiguousarray(coded), codec, 2, 8, src_offset=1)
        want = table.reshape(8, 2).T  # planar
        assert np.array_equal(got.ravel(), np.ascontiguousarray(want).view(np.uint8).ravel()), codec


def check_formats(dev, codec):
    """every out_fmt equals the restatement's conversion of the native result"""
    rng = np.random.default_rng(19)
    cb, fam = R.coded_bytes(codec), R.CODECS[codec][3]
    for ch in (1, 3):
        frames = R.tile_frames(ch, cb, 4) + 7
        b = rng.integers(0, 256, (2, frames * ch * cb), dtype=np.uint8)
        if fam in ("f32", "f64"):  # arbitrary bytes are mostly huge or tiny: half the samples in and around [-1, 1], and the special table
            v = (rng.standard_normal(frames * ch) * 0.9).astype("<f4" if fam == "f32" else "<f8")
            b[0] = v.view(np.uint8)[::1] if codec.endswith("le") else v.view(np.uint8).reshape(-1, cb)[:, ::-1].ravel()
            table = (FLOAT_TABLE_32 if fam == "f32" else F64_FOR_FORMATS).view(np.uint8).reshape(-1, cb)
            b[1, :table.size] = (table if codec.endswith("le") else table[:, ::-1]).ravel()
        shift = top_shift(codec) // 2
        want = R.decode(b, codec, ch, frames, shift)
        for fmt in R.DESTS:
            d_off = R.DEST_BYTES[fmt] if R.DEST_BYTES[fmt] != 3 else 1
            got = run_device(dev, b, codec, ch, frames, shift=shift, fmt=fmt, dst_offset=d_off, pitch_pad=d_off)
            assert np.array_equal(got, R.interleave(want, fam, fmt)), (codec, ch, fmt)


def check_host_equals_resident(dev):
    rng = np.random.default_rng(23)
    for codec, ch, frames, shift in (("s24be", 2, 700, 4), ("alaw", 1, 4097, 0), ("f64le", 3, 95, 0), ("u16le", 8, 300, 15)):
        b = rng.integers(0, 256, (5, frames * ch * R.coded_bytes(codec)), dtype=np.uint8)
        padded = np.concatenate([b, np.full((5, 5), 0x77, np.uint8)], axis=1)  # a host pitch above the packet's bytes
        for fmt in (0, "s16", "u24"):
            res = run_device(dev, b, codec, ch, frames, shift=shift, fmt=fmt)
            pcm = pcm_decode(dev.ctx, padded, codec, ch, frames, shift, fmt if fmt == 0 else FMT[fmt])
            assert np.array_equal(pcm.view(np.uint8).reshape(5, -1), res), (codec, fmt)
    assert pcm_decode(dev.ctx, np.zeros((0, 34), np.uint8), "s16le", 2).shape == (0, 2, 8)
    assert pcm_decode(dev.ctx, np.zeros((3, 3), np.uint8), "s16le", 2).shape == (3, 2, 0)  # fewer bytes than a frame: zero frames, no error


def check_host_chunks(dev):
    """symaccel_pcm_decode cuts where a chunk's coded bytes and output reach 32 MiB, the smallest chunk the context has.
    Whole packets: u8 mono -> native is 2 bytes per frame, 2^20 frames a packet (with a 16-byte multiple as device pitch) is 2 MiB, so a
    chunk holds 16 packets: 17 packets are a chunk and a tail of one.  Frame ranges: one f64 8-channel packet is 128 bytes per frame in
    and out, a chunk is 2^18 frames: 2^18 + 21 frames are a chunk and a tail of 21, whose planes land at the tail's offsets."""
    rng = np.random.default_rng(29)
    b = rng.integers(0, 256, (17, 1 << 20), dtype=np.uint8)
    pcm = pcm_decode(dev.ctx, b, "u8", 1, shift=3)
    assert np.array_equal(pcm[:, 0, :], (b << 3).astype(np.uint8))
    frames = (1 << 18) + 21
    b = rng.integers(0, 256, (1, frames * 64), dtype=np.uint8)
    for fmt in (0, "s16"):
        pcm = pcm_decode(dev.ctx, b, "f64be", 8, out_fmt=fmt if fmt == 0 else FMT[fmt])
        pick = np.r_[0:40, (1 << 18) - 40:frames]
        want = R.decode(b.reshape(1, frames, 64)[:, pick].reshape(1, -1), "f64be", 8, len(pick))
        if fmt == 0:
            assert np.array_equal(pcm[:, :, pick].view(np.uint64), want.view(np.uint64))
            assert np.array_equal(pcm.view(np.uint64)[0].T.ravel(), b.reshape(-1, 8)[:, ::-1].copy().view(np.uint64).ravel())  # (bits moved, all of them)
        else:
            assert np.array_equal(pcm.reshape(frames, 16)[pick].ravel(), R.interleave(want, "f64", "s16").ravel())


def test_kernel_equals_the_reference_fixture(emu_dev):
    check_fixture(emu_dev)


def test_all_twenty_codecs(emu_dev):
    check_all_codecs(emu_dev)


@pytest.mark.parametrize("codec", ("u8", "s16be", "s24le", "f32be", "f64le", "alaw"))
def test_tile_edges_and_channel_counts(emu_dev, codec):
    check_tile_edges(emu_dev, codec)


def test_source_and_output_alignments(emu_dev):
    check_alignments(emu_dev)


def test_packet_counts_and_more_tiles_than_the_grid(emu_dev):
    check_packet_counts(emu_dev, 64)  # (the emulated device has 4 compute units: a grid of 16 workgroups)


def test_float_codecs_move_bits(emu_dev):
    check_float_bits(emu_dev)


@pytest.mark.parametrize("codec", FAMILY_CODECS)
def test_output_formats_equal_the_conversion_of_the_native_result(emu_dev, codec):
    check_formats(emu_dev, codec)


def test_host_to_host_equals_resident(emu_dev):
    check_host_equals_resident(emu_dev)


def test_host_to_host_across_a_chunk_boundary(emu_dev):
    check_host_chunks(emu_dev)


def check_refusals(ctx, src, dst):
    """src / dst: addresses of 4096 / 65536 bytes of (device) memory, dst 16-byte aligned"""
    def status_of(*args):
        with pytest.raises(SymaccelError) as e:
            pcm_decode_device(ctx, *args)
        return e.value.status

    pcm_decode_device(ctx, src, 64, 4, "s16le", 2, 0, 16, dst, 0)  # the baseline is fine
    pcm_decode_device(ctx, src, 64, 4, "s16le", 2, 0, 0, dst, 0)  # zero frames are valid ...
    pcm_decode_device(ctx, src, 0, 4, "s16le", 2, 0, 0, None, 0)  # ... and need no memory
    pcm_decode_device(ctx, src, 64, 0, "s16le", 2, 0, 16, None, 0)
    unsupported = [("s16le", 0, 0), ("s16le", 9, 0), ("s16le", 2, 16), ("u8", 1, 8), ("s24be", 1, 24), ("u32le", 1, 32), ("f32le", 1, 1), ("f64be", 1, 3),
                   ("alaw", 1, 1), ("mulaw", 2, 8)]
    for codec, ch, shift in unsupported:  # the decoder below takes these
        assert status_of(src, 4096, 1, codec, ch, shift, 4, dst, 0) == _ffi.ERR_UNSUPPORTED, (codec, ch, shift)
    bad = [(src, 63, 4, "s16le", 2, 0, 16, dst, 0),  # a pitch below the packet's bytes
           (src, 64, 4, 0, 2, 0, 16, dst, 0), (src, 64, 4, 21, 2, 0, 16, dst, 0),  # unknown codecs
           (src, 64, 4, "s16le", 2, 0, 16, dst, 10), (src, 64, 4, "s16le", 2, 0, 16, dst, -1),  # unknown formats
           (src, 64, 4, "s16le", 2, 17, 16, dst, 0), (src, 64, 4, "u8", 2, 9, 16, dst, 0),  # shifts above the width
           (src, 64, 4, "s16le", 2, 0, 16, dst + 1, 0), (src, 64, 4, "s24le", 1, 0, 16, dst + 2, 0), (src, 128, 4, "f64le", 1, 0, 16, dst + 4, 0),  # alignment
           (src, 64, 4, "s16le", 2, 0, 16, dst + 2, FMT["f32"]), (src, 64, 4, "s16le", 2, 0, 16, dst + 1, FMT["u16"]),
           (None, 64, 4, "s16le", 2, 0, 16, dst, 0), (src, 64, 4, "s16le", 2, 0, 16, None, 0),
           (src, 64, 4, "s16le", 2, 0, 16, src + 64, 0), (src + 64, 64, 4, "s16le", 2, 0, 16, src, 0),  # overlaps
           (src, (1 << 40) + 1, 1, "u8", 1, 0, 16, dst, 0), (src, 64, (1 << 32) + 1, "u8", 1, 0, 16, dst, 0), (src, 1 << 40, 1, "u8", 1, 0, (1 << 36) + 1, dst, 0),
           (src, 1 << 40, 1 << 23, "u8", 1, 0, 16, dst, 0)]  # extents
    for args in bad:
        assert status_of(*args) == _ffi.ERR_INVALID_ARG, args
    pcm_decode_device(ctx, src, 64, 4, "s16le", 2, 0, 16, dst + 1, FMT["s24"])  # the 1- and 3-byte formats go anywhere
    pcm_decode_device(ctx, src, 64, 4, "u8", 2, 0, 16, dst + 3, 0)


def test_refused_shapes_and_bad_arguments(emu_ctx):  # noqa: F811
    src, dst = np.zeros(4096, np.uint8), np.zeros((1 << 16) + 16, np.uint8)
    d = dst.ctypes.data + (-dst.ctypes.data) % 16
    check_refusals(emu_ctx, src.ctypes.data, d)
    assert not dst[(-dst.ctypes.data) % 16 + 400:].any(), "a refused call wrote something"
    for codec, ch, shift in (("s16le", 9, 0), ("alaw", 1, 1)):
        with pytest.raises(SymaccelError) as e:
            pcm_decode(emu_ctx, np.zeros((1, 64), np.uint8), codec, ch, 2, shift)
        assert e.value.status == _ffi.ERR_UNSUPPORTED


# ---- the same on the MI355X --------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_kernel_equals_the_reference_fixture(gpu_dev):
    check_fixture(gpu_dev)


@pytest.mark.gpu
def test_gpu_all_twenty_codecs(gpu_dev):
    check_all_codecs(gpu_dev)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ("u8", "s16be", "s24le", "f32be", "f64le", "alaw"))
def test_gpu_tile_edges_and_channel_counts(gpu_dev, codec):
    check_tile_edges(gpu_dev, codec)


@pytest.mark.gpu
def test_gpu_source_and_output_alignments(gpu_dev):
    check_alignments(gpu_dev)


@pytest.mark.gpu
def test_gpu_packet_counts_and_more_tiles_than_the_grid(gpu_dev):
    check_packet_counts(gpu_dev, 4096)  # (256 compute units, four workgroups each: every workgroup walks four packets)


@pytest.mark.gpu
def test_gpu_float_codecs_move_bits(gpu_dev):
    check_float_bits(gpu_dev)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", FAMILY_CODECS)
def test_gpu_output_formats_equal_the_conversion_of_the_native_result(gpu_dev, codec):
    check_formats(gpu_dev, codec)


@pytest.mark.gpu
def test_gpu_host_to_host_equals_resident(gpu_dev):
    check_host_equals_resident(gpu_dev)


@pytest.mark.gpu
def test_gpu_host_to_host_across_a_chunk_boundary(gpu_dev):
    check_host_chunks(gpu_dev)


@pytest.mark.gpu
def test_gpu_refused_shapes_and_bad_arguments(gpu_dev):
    src, dst = gpu_dev.zeros(4096), gpu_dev.zeros((1 << 16) + 16)
    check_refusals(gpu_dev.ctx, gpu_dev.addr(src), gpu_dev.addr(dst) + (-gpu_dev.addr(dst)) % 16)
    assert not gpu_dev.get(dst)[(-gpu_dev.addr(dst)) % 16 + 400:].any(), "a refused call wrote something"


@pytest.mark.gpu
def test_gpu_byte_tables():
    from symphonia_amd import default_library
    lib = default_library()
    for name in R.NAMES:
        assert pcm_coded_bytes(name, lib) == R.coded_bytes(name) and pcm_native_bytes(name, lib) == R.native_bytes(name)
    assert lib.dll.symaccel_abi_version() == 8
