"""ADPCM on the device: symaccel_adpcm_decode(_device) against symphonia-codec-adpcm's block decoders (codec_ms.rs, codec_ima_wav.rs,
codec_ima_qt.rs; mono and stereo).

Expected samples come from two independent places that must agree:
  * tests/golden/adpcm.npz -- the reference's decode_mono / decode_stereo executed under tools/rsinterp (tools/make_adpcm_fixtures.py; the
    localref case below regenerates it from the reference tree and compares): encoder packets, hand-made edge blocks, arbitrary bytes,
    and arbitrary MS bytes on which the reference's release build wraps (recorded with the interpreter's count of wraps);
  * tests/adpcm_ref.py -- a numpy restatement with the wrapping written out, pinned to the fixture bit for bit, and to a scalar form
    of itself.
The kernel is checked against the fixture on the fixture's blocks and against the restatement on arbitrary bytes for every shape at which
it takes another path: header-only blocks, a last step that is not full, blocks longer than one 64-byte piece, block counts that do not fill
a 64-block tile, more tiles than the grid holds, pitches and bases of every alignment.  Every comparison is on bytes, no tolerance.  CPU
emulation here, gpu-marked twins on the MI355X."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from emu_lib import emu_ctx, emu_library  # noqa: F401
from symphonia_amd import (ADPCM_IMA_QT, ADPCM_IMA_WAV, ADPCM_MS, Context, SymaccelError, adpcm_block_bytes, adpcm_decode, adpcm_decode_device)
from symphonia_amd import _ffi
from test_pcm_convert import BYTES, FMT, EmuDev, GpuDev, expected

import adpcm_ref as R

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
GOLDEN = ROOT / "tests" / "golden" / "adpcm.npz"
GUARD = 0xA5
CODEC = {"ms": ADPCM_MS, "ima_wav": ADPCM_IMA_WAV, "ima_qt": ADPCM_IMA_QT}
KINDS = [(c, ch) for c in ("ms", "ima_wav", "ima_qt") for ch in (1, 2)]
KIND_IDS = ["%s_%d" % k for k in KINDS]
# frames per block: the preamble alone; one step (16 nibbles) short, exact and one over; the data of exactly one 64-byte piece, one byte
# over, several pieces
ACCEPTED = {("ms", 1): (2, 4, 18, 20, 130, 132, 300), ("ms", 2): (2, 3, 10, 11, 66, 67, 203), ("ima_wav", 1): (1, 3, 17, 19, 129, 131, 301),
            ("ima_wav", 2): (1, 9, 17, 65, 73, 201), ("ima_qt", 1): (64,), ("ima_qt", 2): (64,)}
REFUSED = [("ms", 1, 0), ("ms", 1, 1), ("ms", 2, 1), ("ms", 1, 3), ("ms", 1, 133), ("ima_wav", 1, 0), ("ima_wav", 1, 2), ("ima_wav", 1, 130),
           ("ima_wav", 2, 0), ("ima_wav", 2, 2), ("ima_wav", 2, 10), ("ima_wav", 2, 64), ("ima_qt", 1, 63), ("ima_qt", 2, 65), ("ima_qt", 1, 128),
           ("ms", 3, 20), ("ima_wav", 0, 9), ("ima_qt", 3, 64), ("ms", 2, (1 << 20) + 1)]


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


def arbitrary(rng, codec, channels, fpb, n, bad_every=0):
    """n blocks of arbitrary bytes whose preambles the reference accepts, except every `bad_every`-th"""
    b = rng.integers(0, 256, (n, R.block_bytes(CODEC[codec], channels, fpb)), dtype=np.uint8)
    if codec == "ms":
        b[:, :channels] %= 7
        if bad_every:
            b[1::bad_every, channels - 1] = 7 + b[1::bad_every, 3] % 249
    elif codec == "ima_wav":
        for c in range(channels):
            b[:, 4 * c + 2] %= 89
        if bad_every:
            b[1::bad_every, 4 * (channels - 1) + 2] = 89 + b[1::bad_every, 0] % 167
    return b


def run_device(dev, blocks, codec, channels, fpb, fmt=0, pitch_pad=0, src_offset=0, dst_offset=0):
    """symaccel_adpcm_decode_device on blocks laid out at block bytes + pitch_pad, the first one src_offset bytes past an aligned address;
    -> (pcm bytes uint8[n, bytes of a block's output], status uint8[n]); checks that nothing outside the two outputs was written"""
    n, nb = blocks.shape
    pitch = nb + pitch_pad
    rows = np.full((n, pitch), 0x5A, np.uint8)
    rows[:, :nb] = blocks
    src = np.concatenate([np.full(src_offset, 0x5A, np.uint8), rows.ravel()[:max(n - 1, 0) * pitch + nb]])  # (the last block ends the buffer: nothing behind it may be read)
    ob = channels * fpb * (4 if fmt == 0 else BYTES[fmt])
    d_src, d_dst, d_st = dev.put(src), dev.zeros(dst_offset + n * ob + 64, GUARD), dev.zeros(16 + n + 48, GUARD)
    adpcm_decode_device(dev.ctx, dev.addr(d_src) + src_offset, pitch, n, CODEC[codec], channels, fpb, dev.addr(d_dst) + dst_offset, 0 if fmt == 0 else FMT[fmt],
                        dev.addr(d_st) + 16)
    out, st = dev.get(d_dst), dev.get(d_st)
    assert np.all(out[:dst_offset] == GUARD) and np.all(out[dst_offset + n * ob:] == GUARD), "bytes outside the PCM were written"
    assert np.all(st[:16] == GUARD) and np.all(st[16 + n:] == GUARD), "bytes outside the status array were written"
    return out[dst_offset:dst_offset + n * ob].reshape(n, ob), st[16:16 + n]


def native(pcm_bytes, channels, fpb):
    return np.ascontiguousarray(pcm_bytes).view(np.int32).reshape(-1, channels, fpb)


def fixture():
    z = np.load(GOLDEN)
    return z, json.loads(bytes(z["manifest"]).decode())["entries"]


# ---- the two expectations agree --------------------------------------------------------------------------------------------------------

def test_restatement_equals_the_reference_fixture():
    z, entries = fixture()
    assert {(e["codec"], e["channels"]) for e in entries} == set(KINDS)
    for e in entries:
        pcm, status = R.decode(z[e["name"] + "_bytes"], e["codec"], e["channels"], e["frames_per_block"])
        assert np.array_equal(pcm, z[e["name"] + "_pcm"]) and not status.any(), e["name"]


def test_fixture_holds_the_wrapping_case_and_only_there():
    _, entries = fixture()
    for e in entries:
        assert (e["overflows"] > 0) == e["name"].startswith("wrap_ms_"), e


@pytest.mark.parametrize("codec,channels", KINDS, ids=KIND_IDS)
def test_vectorised_restatement_equals_its_scalar_form(codec, channels):
    rng = np.random.default_rng(5)
    for fpb in ACCEPTED[(codec, channels)][-3:]:
        b = arbitrary(rng, codec, channels, fpb, 4, bad_every=3)
        pcm, status = R.decode(b, codec, channels, fpb)
        for i in range(len(b)):
            one, code = R.decode_scalar(b[i], codec, channels, fpb)
            assert code == status[i]
            assert np.array_equal(pcm[i], one) if code == 0 else not pcm[i].any()


@pytest.mark.localref
def test_fixture_regenerates_from_the_reference_tree():
    import make_adpcm_fixtures as M
    assert M.compare(M.generate(), dict(np.load(GOLDEN))) == []


def test_block_bytes_table():
    lib = emu_library()
    for (codec, ch), fpbs in ACCEPTED.items():
        for fpb in fpbs:
            assert adpcm_block_bytes(codec, ch, fpb, lib) == R.block_bytes(CODEC[codec], ch, fpb) > 0
    assert [adpcm_block_bytes("ms", 1, 2036, lib), adpcm_block_bytes("ms", 2, 1012, lib), adpcm_block_bytes("ima_wav", 1, 1017, lib),
            adpcm_block_bytes("ima_wav", 2, 505, lib), adpcm_block_bytes("ima_qt", 1, 64, lib), adpcm_block_bytes("ima_qt", 2, 64, lib)] == [1024, 1024, 512, 512, 34, 68]
    for codec, ch, fpb in REFUSED:
        assert adpcm_block_bytes(codec, ch, fpb, lib) == 0, (codec, ch, fpb)
    assert adpcm_block_bytes(0, 1, 64, lib) == 0 and adpcm_block_bytes(4, 2, 64, lib) == 0
    assert (ADPCM_MS, ADPCM_IMA_WAV, ADPCM_IMA_QT) == (1, 2, 3)


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------

def check_fixture(dev):
    z, entries = fixture()
    for e in entries:
        got, status = run_device(dev, z[e["name"] + "_bytes"], e["codec"], e["channels"], e["frames_per_block"])
        assert np.array_equal(native(got, e["channels"], e["frames_per_block"]), z[e["name"] + "_pcm"]) and not status.any(), e["name"]


def check_arbitrary(dev, codec, channels):
    """every accepted shape; 67 blocks (a full tile and a partial one), pitches and bases of every alignment class, every third block
    with a preamble the reference rejects"""
    rng = np.random.default_rng(17)
    for k, fpb in enumerate(ACCEPTED[(codec, channels)]):
        b = arbitrary(rng, codec, channels, fpb, 67, bad_every=3)
        want, want_status = R.decode(b, codec, channels, fpb)
        if codec != "ima_qt":
            assert want_status[1::3].all() and not want_status[0::3].any() and not want_status[2::3].any()
            assert not want[1::3].any() and want[0::3].any()
        for pad, s_off, d_off in ((0, 0, 0), ((3, 16, 1, 29)[k % 4], (1, 15, 8, 2)[k % 4], (4, 12, 8, 4)[k % 4])):
            got, status = run_device(dev, b, codec, channels, fpb, pitch_pad=pad, src_offset=s_off, dst_offset=d_off)
            assert np.array_equal(status, want_status), (fpb, pad)
            assert np.array_equal(native(got, channels, fpb), want), (fpb, pad, s_off, d_off)


def check_block_counts(dev):
    rng = np.random.default_rng(23)
    for codec, ch, fpb in (("ms", 2, 35), ("ima_wav", 1, 41), ("ima_qt", 2, 64)):
        for n in (1, 2, 63, 64, 65, 129):
            b = arbitrary(rng, codec, ch, fpb, n)
            got, status = run_device(dev, b, codec, ch, fpb, src_offset=n % 16)
            assert np.array_equal(native(got, ch, fpb), R.decode(b, codec, ch, fpb)[0]) and not status.any(), (codec, n)


def check_formats(dev, codec, channels):
    """every output format equals the conversion of the native result (tests/test_pcm_convert.py: the restatement pinned to conv.rs),
    a block being the interleave group; bad blocks are the format's silence"""
    rng = np.random.default_rng(29)
    fpb = ACCEPTED[(codec, channels)][-2 if codec != "ima_qt" else 0]
    b = arbitrary(rng, codec, channels, fpb, 66, bad_every=5)
    want, _ = R.decode(b, codec, channels, fpb)
    planes = want.reshape(len(b) * channels, fpb)
    for fmt in FMT:
        for d_off in (0, BYTES[fmt] if BYTES[fmt] != 3 else 1):
            got, _ = run_device(dev, b, codec, channels, fpb, fmt=fmt, dst_offset=d_off, pitch_pad=d_off)
            assert np.array_equal(got, expected("s32", fmt, planes, channels, fpb)), (fmt, d_off)


def check_many_tiles(dev, n):
    """more tiles than the grid holds: a workgroup walks several"""
    rng = np.random.default_rng(31)
    b = arbitrary(rng, "ima_qt", 1, 64, n)
    got, status = run_device(dev, b, "ima_qt", 1, 64, fmt="s16")
    want, _ = R.decode(b, "ima_qt", 1, 64)
    assert np.array_equal(got.view(np.int16), (want[:, 0, :] >> 16).astype(np.int16)) and not status.any()


def check_host_equals_resident(dev):
    rng = np.random.default_rng(37)
    for codec, ch, fpb in (("ms", 1, 300), ("ima_wav", 2, 201), ("ima_qt", 2, 64)):
        b = arbitrary(rng, codec, ch, fpb, 70, bad_every=4)
        padded = np.concatenate([b, np.full((len(b), 5), 0x77, np.uint8)], axis=1)  # a host pitch above the block's bytes
        for fmt in (0, "s16", "u24"):
            res, res_status = run_device(dev, b, codec, ch, fpb, fmt=fmt)
            pcm, status = adpcm_decode(dev.ctx, padded, codec, ch, fpb, fmt if fmt == 0 else FMT[fmt])
            assert np.array_equal(pcm.view(np.uint8).reshape(len(b), -1), res) and np.array_equal(status, res_status), (codec, fmt)
    pcm, status = adpcm_decode(dev.ctx, np.zeros((0, 34), np.uint8), "ima_qt", 1, 64)
    assert pcm.shape == (0, 1, 64) and status.shape == (0,)


def check_host_in_two_chunks(dev):
    """symaccel_adpcm_decode cuts its batch where a chunk's blocks and their output reach 32 MiB.  MS stereo at 1012 frames per block
    is 1024 bytes in and 8096 out (native i32), so a chunk holds floor(32 MiB / (1024 + 8096)) = 3679 blocks; 3679 + 5 blocks are a full
    chunk and a tail of 5, whose blocks, PCM and status bytes sit at the second chunk's offsets into the caller's arrays.  Every third
    block is bad, so the status bytes differ on both sides of the cut.  Expected: the resident result on the same bytes, and the
    restatement for blocks on both sides of the cut."""
    codec, ch, fpb, cut = "ms", 2, 1012, 3679
    assert R.block_bytes(CODEC[codec], ch, fpb) == 1024 and (32 << 20) // (1024 + ch * fpb * 4) == cut
    n = cut + 5
    b = arbitrary(np.random.default_rng(41), codec, ch, fpb, n, bad_every=3)
    padded = np.concatenate([b, np.full((n, 5), 0x77, np.uint8)], axis=1)  # a host pitch above the block's bytes
    res, res_status = run_device(dev, b, codec, ch, fpb)
    pcm, status = adpcm_decode(dev.ctx, padded, codec, ch, fpb)
    assert np.array_equal(status, res_status) and np.array_equal(pcm.view(np.uint8).reshape(n, -1), res)
    pick = np.r_[0:3, cut - 4:n]
    want, want_status = R.decode(b[pick], codec, ch, fpb)
    assert want_status[pick < cut].any() and want_status[pick >= cut].any() and not want_status[pick >= cut].all()
    assert np.array_equal(status[pick], want_status) and np.array_equal(pcm[pick], want)


def test_kernel_equals_the_reference_fixture(emu_dev):
    check_fixture(emu_dev)


@pytest.mark.parametrize("codec,channels", KINDS, ids=KIND_IDS)
def test_kernel_equals_restatement_on_arbitrary_bytes(emu_dev, codec, channels):
    check_arbitrary(emu_dev, codec, channels)


def test_block_counts_that_do_not_fill_a_tile(emu_dev):
    check_block_counts(emu_dev)


@pytest.mark.parametrize("codec,channels", KINDS, ids=KIND_IDS)
def test_output_formats_equal_pcm_convert_of_the_native_result(emu_dev, codec, channels):
    check_formats(emu_dev, codec, channels)


def test_more_tiles_than_the_grid(emu_dev):
    check_many_tiles(emu_dev, 64 * 41 + 5)  # (the emulated device has 4 compute units: a grid of 40 workgroups)


def test_host_to_host_equals_resident(emu_dev):
    check_host_equals_resident(emu_dev)


def test_host_to_host_in_two_chunks_equals_resident(emu_dev):
    check_host_in_two_chunks(emu_dev)


def test_refused_shapes_and_bad_arguments(emu_ctx):  # noqa: F811
    ctx = emu_ctx
    src, dst, st = np.zeros(4096, np.uint8), np.zeros(1 << 16, np.uint8), np.zeros(64, np.uint8)
    s, d, t = src.ctypes.data, dst.ctypes.data, st.ctypes.data

    def status_of(*args):
        with pytest.raises(SymaccelError) as e:
            adpcm_decode_device(ctx, *args)
        return e.value.status

    adpcm_decode_device(ctx, s, 34, 4, "ima_qt", 1, 64, d, 0, t)  # the baseline is fine
    adpcm_decode_device(ctx, s, 34, 4, "ima_qt", 1, 64, d, 0, None)  # the status array is optional
    adpcm_decode_device(ctx, s, 34, 0, "ima_qt", 1, 64, None, 0, None)  # nothing to do is not an error
    for codec, ch, fpb in REFUSED:  # the decoder below takes these
        assert status_of(s, 4096, 1, codec, ch, fpb, d, 0, t) == _ffi.ERR_UNSUPPORTED, (codec, ch, fpb)
        with pytest.raises(SymaccelError) as e:
            adpcm_decode(ctx, np.zeros((1, 4096), np.uint8), codec, ch, fpb)
        assert e.value.status == _ffi.ERR_UNSUPPORTED
    bad = [(s, 33, 4, "ima_qt", 1, 64, d, 0, t),        # a pitch below the block's bytes
           (s, 34, 4, 0, 1, 64, d, 0, t), (s, 34, 4, 4, 1, 64, d, 0, t),  # unknown codecs
           (s, 34, 4, "ima_qt", 1, 64, d, 10, t), (s, 34, 4, "ima_qt", 1, 64, d, -1, t),  # unknown formats
           (s, 34, 4, "ima_qt", 1, 64, d + 2, 0, t), (s, 34, 4, "ima_qt", 1, 64, d + 1, FMT["s16"], t), (s, 34, 4, "ima_qt", 1, 64, d + 2, FMT["f32"], t),  # alignment
           (None, 34, 4, "ima_qt", 1, 64, d, 0, t), (s, 34, 4, "ima_qt", 1, 64, None, 0, t),
           (s, 34, 4, "ima_qt", 1, 64, s + 64, 0, t), (s, 34, 4, "ima_qt", 1, 64, d, 0, d + 100), (s, 34, 4, "ima_qt", 1, 64, d, 0, s + 3),  # overlaps
           (s, (1 << 24) + 1, 1, "ima_qt", 1, 64, d, 0, t), (s, 34, (1 << 32) + 1, "ima_qt", 1, 64, d, 0, t)]
    for args in bad:
        assert status_of(*args) == _ffi.ERR_INVALID_ARG, args
    adpcm_decode_device(ctx, s, 34, 4, "ima_qt", 1, 64, d + 1, FMT["s24"], t)  # the 1- and 3-byte formats go anywhere
    assert not dst[4 * 64 * 4 + 8:].any(), "a refused call wrote something"


# ---- the same on the MI355X --------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_kernel_equals_the_reference_fixture(gpu_dev):
    check_fixture(gpu_dev)


@pytest.mark.gpu
@pytest.mark.parametrize("codec,channels", KINDS, ids=KIND_IDS)
def test_gpu_kernel_equals_restatement_on_arbitrary_bytes(gpu_dev, codec, channels):
    check_arbitrary(gpu_dev, codec, channels)


@pytest.mark.gpu
def test_gpu_block_counts_that_do_not_fill_a_tile(gpu_dev):
    check_block_counts(gpu_dev)


@pytest.mark.gpu
@pytest.mark.parametrize("codec,channels", KINDS, ids=KIND_IDS)
def test_gpu_output_formats_equal_pcm_convert_of_the_native_result(gpu_dev, codec, channels):
    check_formats(gpu_dev, codec, channels)


@pytest.mark.gpu
def test_gpu_more_tiles_than_the_grid(gpu_dev):
    check_many_tiles(gpu_dev, 64 * 2560 * 2 + 77)  # (256 compute units, ten workgroups each: every workgroup walks two tiles and some a third)


@pytest.mark.gpu
def test_gpu_host_to_host_equals_resident(gpu_dev):
    check_host_equals_resident(gpu_dev)


@pytest.mark.gpu
def test_gpu_host_to_host_in_two_chunks_equals_resident(gpu_dev):
    check_host_in_two_chunks(gpu_dev)


@pytest.mark.gpu
def test_gpu_block_bytes_table():
    from symphonia_amd import default_library
    lib = default_library()
    for codec, ch, fpb in REFUSED:
        assert adpcm_block_bytes(codec, ch, fpb, lib) == 0
    assert adpcm_block_bytes("ms", 2, 1012, lib) == 1024 and adpcm_block_bytes("ima_qt", 2, 64, lib) == 68
