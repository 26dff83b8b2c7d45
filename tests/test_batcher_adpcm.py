"""The batcher's ninth kind, SYMACCEL_BATCH_ADPCM_DECODE: a chain is one ADPCM block, units_per_chain its bytes, param = codec | channels << 8
(symphonia-codec-adpcm lib.rs:122-168: a packet is blocks back to back, and no state passes from one to the next).  Packets of many
streams of mixed codecs and shapes share launches; every result equals the per-stream call and the numpy restatement (tests/adpcm_ref.py,
pinned to the reference fixture by tests/test_adpcm.py); a packet with a block the reference rejects fails alone with the reference's
error class; an output format is delivered by the decode kernel itself, a block's channels being the interleave group; the statistics of
other kinds are what they are without ADPCM beside them.  CPU emulation here, gpu-marked twins on the MI355X."""
import numpy as np
import pytest

from emu_lib import emu_ctx, emu_library  # noqa: F401
from symphonia_amd import (BATCH_ADPCM_DECODE, FLAC_VERBATIM, Batcher, Context, SymaccelError, adpcm_decode, flac_desc)
from symphonia_amd import _ffi
from test_pcm_convert import BYTES, FMT, expected

import adpcm_ref as R

SHAPES = [("ms", 2, 35), ("ima_wav", 1, 41), ("ima_qt", 2, 64), ("ms", 1, 132), ("ima_wav", 2, 73), ("ima_qt", 1, 64)]


def param(codec, ch):
    return R.CODECS[codec] | ch << 8


def packet(rng, codec, ch, fpb, n):
    b = rng.integers(0, 256, (n, R.block_bytes(R.CODECS[codec], ch, fpb)), dtype=np.uint8)
    if codec == "ms":
        b[:, :ch] %= 7
    elif codec == "ima_wav":
        for c in range(ch):
            b[:, 4 * c + 2] %= 89
    return b


@pytest.fixture(scope="module")
def gpu_ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on an MI355X (there is no CPU path)")
    ctx = Context(0)
    yield ctx
    ctx.close()


def check_sharing(ctx):
    rng = np.random.default_rng(41)
    b = Batcher(ctx)
    subs = []
    for s in range(30):  # thirty streams, six shapes, packets of one to seven blocks
        codec, ch, fpb = SHAPES[s % len(SHAPES)]
        blocks = packet(rng, codec, ch, fpb, 1 + s % 7)
        out = np.zeros((len(blocks), ch, fpb), np.int32)
        subs.append((b.submit_adpcm_decode(blocks, codec, ch, out), blocks, codec, ch, fpb, out))
    assert b.stats()["pending"] == 30
    for t, blocks, codec, ch, fpb, out in subs:
        b.collect(t)
        assert np.array_equal(out, R.decode(blocks, codec, ch, fpb)[0]), (codec, ch)
    st = b.stats()
    assert st["launches"] == len(SHAPES) < st["submissions"] == 30 and st["failed_tickets"] == 0, st
    assert st["chains_launched"] == sum(1 + s % 7 for s in range(30))
    b.close()
    for t, blocks, codec, ch, fpb, out in subs[:6]:  # the per-stream entry point gives the same
        pcm, status = adpcm_decode(ctx, blocks, codec, ch, fpb)
        assert np.array_equal(pcm, out) and not status.any()
    return st


def check_bad_block(ctx):
    rng = np.random.default_rng(43)
    b = Batcher(ctx)
    failing = []
    for codec, ch, fpb, at, value, status in (("ms", 2, 35, 1, 7, _ffi.ERR_UNSUPPORTED), ("ms", 1, 132, 0, 255, _ffi.ERR_UNSUPPORTED),
                                              ("ima_wav", 1, 41, 2, 89, _ffi.ERR_DECODE), ("ima_wav", 2, 73, 6, 200, _ffi.ERR_DECODE)):
        failed = b.stats()["failed_tickets"]
        packets = [packet(rng, codec, ch, fpb, n) for n in (3, 4, 2)]
        packets[1][2, at] = value  # the third block of the second packet
        outs = [np.zeros((len(p), ch, fpb), np.int32) for p in packets]
        tickets = [b.submit_adpcm_decode(p, codec, ch, o) for p, o in zip(packets, outs)]
        b.collect(tickets[0])
        with pytest.raises(SymaccelError) as e:
            b.collect(tickets[1])
        assert e.value.status == status, (codec, ch)
        failing.append((packets[1], codec, ch, fpb, status))
        b.collect(tickets[2])
        for i in (0, 2):
            assert np.array_equal(outs[i], R.decode(packets[i], codec, ch, fpb)[0])
        assert b.stats()["failed_tickets"] == failed + 1
    # both errors in one packet: the first bad block decides, as the reference stops there
    p = packet(rng, "ima_wav", 1, 41, 3)
    p[1, 2] = 120
    t = b.submit_adpcm_decode(p, "ima_wav", 1, np.zeros((3, 1, 41), np.int32))
    with pytest.raises(SymaccelError) as e:
        b.collect(t)
    assert e.value.status == _ffi.ERR_DECODE
    b.close()
    # the batcher reads the preambles on the host (csrc/batcher.cpp check_adpcm): it must say what the kernel's status bytes say
    for blocks, codec, ch, fpb, status in failing:
        kernel_status = adpcm_decode(ctx, blocks, codec, ch, fpb)[1]
        assert kernel_status.nonzero()[0].tolist() == [2] and {1: _ffi.ERR_UNSUPPORTED, 2: _ffi.ERR_DECODE}[int(kernel_status[2])] == status


def check_formats(ctx):
    rng = np.random.default_rng(47)
    b = Batcher(ctx)
    subs = []
    for k, fmt in enumerate(FMT):
        codec, ch, fpb = SHAPES[k % 3]
        blocks = packet(rng, codec, ch, fpb, 2 + k % 3)
        out = np.zeros((len(blocks), fpb * ch * BYTES[fmt]), np.uint8)
        subs.append((b.submit_adpcm_decode(blocks, codec, ch, out, out_format=fmt), blocks, codec, ch, fpb, out, fmt))
    for t, blocks, codec, ch, fpb, out, fmt in subs:
        b.collect(t)
        planes = R.decode(blocks, codec, ch, fpb)[0].reshape(len(blocks) * ch, fpb)
        assert np.array_equal(out, expected("s32", fmt, planes, ch, fpb)), (codec, fmt)
    # the zero-copy form: out_bytes is the converted size from reserve() on
    blocks = packet(rng, "ms", 2, 35, 5)
    t, slot = b.reserve(BATCH_ADPCM_DECODE, param("ms", 2), 5, blocks.shape[1], out_format="s16", channels=2)
    assert slot.input_bytes[0] == blocks.size and slot.out_bytes == 5 * 35 * 2 * 2
    np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * blocks.size).from_address(slot.input[0]))[:] = blocks.ravel()
    b.commit(t)
    slot = b.wait(t)
    got = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_int16 * (5 * 35 * 2)).from_address(slot.out)).reshape(5, 35, 2).copy()
    b.release(t)
    assert np.array_equal(got, (R.decode(blocks, "ms", 2, 35)[0] >> 16).astype(np.int16).transpose(0, 2, 1))
    for bad in ((param("ms", 2), 5, 47, "s16", 1), (param("ms", 2), 5, 47, 10, 2), (param("ms", 2) | 4 << 16, 5, 47, "s16", 2)):  # channels, format, a format inside param
        with pytest.raises(SymaccelError) as e:
            b.reserve(BATCH_ADPCM_DECODE, bad[0], bad[1], bad[2], out_format=bad[3], channels=bad[4])
        assert e.value.status == _ffi.ERR_INVALID_ARG
    st = b.stats()
    b.close()
    return st


def check_reserve_refusals(ctx):
    b = Batcher(ctx)
    for codec, ch, units in (("ms", 1, 6), ("ms", 2, 13), ("ima_wav", 1, 3), ("ima_wav", 2, 9), ("ima_wav", 2, 7), ("ima_qt", 1, 35), ("ima_qt", 2, 34), ("ms", 3, 64),
                             ("ms", 0, 64)):
        with pytest.raises(SymaccelError) as e:
            b.reserve(BATCH_ADPCM_DECODE, param(codec, ch), 2, units)
        assert e.value.status == _ffi.ERR_INVALID_ARG, (codec, ch, units)
    for p in (0, 4 | 1 << 8, param("ms", 1) | 1 << 16, -1):
        with pytest.raises(SymaccelError):
            b.reserve(BATCH_ADPCM_DECODE, p, 2, 34)
    t, slot = b.reserve(BATCH_ADPCM_DECODE, param("ima_wav", 2), 3, 8)  # the smallest stereo block: the preambles alone
    assert slot.out_bytes == 3 * 2 * 1 * 4
    b.release(t)
    assert b.stats()["failed_tickets"] == 0
    b.close()


def flac_rounds(ctx, with_adpcm):
    """three FLAC_RESTORE submissions per round, two rounds; optionally ADPCM packets between them -> the batcher's counters"""
    rng = np.random.default_rng(53)
    arng = np.random.default_rng(59)
    b = Batcher(ctx)
    for _ in range(2):
        subs, extra = [], []
        for s in range(3):
            buf = rng.integers(-1000, 1000, (2 + s, 64)).astype(np.int32)
            got = buf.copy()
            desc = np.ascontiguousarray(flac_desc(np.full(len(buf), FLAC_VERBATIM), np.zeros(len(buf)), np.zeros(len(buf)), np.zeros(len(buf))))
            subs.append((b.submit_flac_restore(got, desc, np.zeros((len(buf), 32), np.int32)), got, buf))
            if with_adpcm:
                blocks = packet(arng, "ima_qt", 2, 64, 3)
                out = np.zeros((3, 2, 64), np.int32)
                extra.append((b.submit_adpcm_decode(blocks, "ima_qt", 2, out), blocks, out))
        for t, got, want in subs:
            b.collect(t)
            assert np.array_equal(got, want)
        for t, blocks, out in extra:
            b.collect(t)
            assert np.array_equal(out, R.decode(blocks, "ima_qt", 2, 64)[0])
    st = b.stats()
    b.close()
    return {k: st[k] for k in ("submissions", "launches", "chunks", "chains_launched", "max_chains_per_launch", "failed_tickets")}


def check_other_kinds_unchanged(ctx):
    alone, mixed = flac_rounds(ctx, False), flac_rounds(ctx, True)
    assert alone == {"submissions": 6, "launches": 2, "chunks": 2, "chains_launched": 18, "max_chains_per_launch": 9, "failed_tickets": 0}, alone
    # beside ADPCM: the FLAC groups are launched as before, the ADPCM packets add one launch of 9 blocks per round
    assert mixed == {"submissions": 12, "launches": 4, "chunks": 4, "chains_launched": 36, "max_chains_per_launch": 9, "failed_tickets": 0}, mixed


def test_streams_of_mixed_codecs_share_launches(emu_ctx):  # noqa: F811
    check_sharing(emu_ctx)


def test_a_bad_block_fails_its_ticket_alone(emu_ctx):  # noqa: F811
    check_bad_block(emu_ctx)


def test_output_formats_through_the_batcher(emu_ctx):  # noqa: F811
    check_formats(emu_ctx)


def test_byte_counts_without_a_shape_fail_at_reserve(emu_ctx):  # noqa: F811
    check_reserve_refusals(emu_ctx)


def test_statistics_of_other_kinds_are_unchanged_beside_adpcm(emu_ctx):  # noqa: F811
    check_other_kinds_unchanged(emu_ctx)


def test_kind_value_and_plane_bytes():
    assert BATCH_ADPCM_DECODE == 9
    lib = emu_library()
    import ctypes as C
    ins, sts, out = (C.c_size_t * 6)(), (C.c_size_t * 3)(), C.c_size_t()
    assert lib.dll.symaccel_batcher_plane_bytes(BATCH_ADPCM_DECODE, param("ms", 2), 1024, ins, sts, C.byref(out)) == 0
    assert list(ins) == [1024, 0, 0, 0, 0, 0] and list(sts) == [0, 0, 0] and out.value == 2 * 1012 * 4
    assert lib.dll.symaccel_batcher_plane_bytes(BATCH_ADPCM_DECODE, param("ima_wav", 1), 5, ins, sts, C.byref(out)) == 0 and out.value == 3 * 4
    assert lib.dll.symaccel_batcher_plane_bytes(BATCH_ADPCM_DECODE, param("ima_wav", 2), 9, ins, sts, C.byref(out)) == _ffi.ERR_INVALID_ARG


@pytest.mark.gpu
def test_gpu_streams_of_mixed_codecs_share_launches(gpu_ctx):
    check_sharing(gpu_ctx)


@pytest.mark.gpu
def test_gpu_a_bad_block_fails_its_ticket_alone(gpu_ctx):
    check_bad_block(gpu_ctx)


@pytest.mark.gpu
def test_gpu_output_formats_through_the_batcher(gpu_ctx):
    check_formats(gpu_ctx)


@pytest.mark.gpu
def test_gpu_statistics_of_other_kinds_are_unchanged_beside_adpcm(gpu_ctx):
    check_other_kinds_unchanged(gpu_ctx)
