"""The batcher's tenth kind, SYMACCEL_BATCH_MPA12_DECODE: a chain is a channel, units_per_chain the packets, param the layer.  Ragged
groups of mono and stereo submissions of both layers share launches; every result equals the per-stream entry point
(symaccel_mpa12_decode) and the reference arithmetic (tests/mpa12_ref.py + the oracle's polyphase), bit for bit; groups cut into many
chunks give the same; a submission with a record out of range fails alone and runs as silence; an output format is what
symaccel_pcm_convert makes of the native planes.  CPU emulation here, gpu-marked twins on the MI355X."""
import ctypes as C

import numpy as np
import pytest

import mpa12_ref as R
from emu_lib import emu_ctx, emu_library  # noqa: F401
from helpers import bit_equal
from symphonia_amd import BATCH_MPA12_DECODE, Batcher, Context, Mpa12Decode, SymaccelError, _ffi, pcm_convert
from test_mpa12 import case


@pytest.fixture(scope="module")
def gpu_ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on an MI355X (there is no CPU path)")
    ctx = Context(0)
    yield ctx
    ctx.close()


def submit(b, layer, inputs):
    """the copy form; returns (ticket, the arrays collect() fills)"""
    codes, rec, vvec, vfront = inputs
    vv, vf = vvec.copy(), vfront.copy()
    pcm = np.full(codes.shape[:2] + (32 * R.N_FRAMES[layer],), np.nan, np.float32)
    return b.submit(BATCH_MPA12_DECODE, layer, [np.ascontiguousarray(codes), np.ascontiguousarray(rec)], [vv, vf], pcm), (pcm, vv, vf)


# (layer, channels, packets): two unit counts per layer, so four groups; mono and stereo streams side by side in each
STREAMS = [(R.LAYER1, 1, 2), (R.LAYER2, 2, 1), (R.LAYER1, 2, 2), (R.LAYER2, 1, 6), (R.LAYER1, 3, 9), (R.LAYER2, 2, 6), (R.LAYER1, 1, 9),
           (R.LAYER2, 1, 1), (R.LAYER1, 2, 9), (R.LAYER2, 3, 6), (R.LAYER1, 3, 2), (R.LAYER2, 3, 1)]


def check_sharing(ctx):
    b = Batcher(ctx)
    subs = []
    for layer, nch, npk in STREAMS:
        inputs, want = case(layer, nch, npk)
        subs.append((submit(b, layer, inputs), layer, inputs, want))
    assert b.stats()["pending"] == len(STREAMS)
    for (t, got), layer, inputs, want in subs:
        b.collect(t)
        assert bit_equal(got[0], want[0]) and bit_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (layer, inputs[0].shape)
    st = b.stats()
    assert st["launches"] == 4 < st["submissions"] == len(STREAMS) and st["failed_tickets"] == 0, st
    assert st["chains_launched"] == sum(s[1] for s in STREAMS)
    b.close()
    for (t, got), layer, inputs, want in subs[:4]:  # the per-stream entry point gives the same
        pcm, vv, vf, status = Mpa12Decode(ctx, layer).decode(*inputs)
        assert bit_equal(pcm, got[0]) and bit_equal(vv, got[1]) and np.array_equal(vf, got[2]) and not status.any()
    return st


def check_many_chunks(ctx):
    """one group of 40 stereo Layer II submissions of 6 packets (28.5 KiB of input each): 64 KiB chunks hold two of them"""
    b = Batcher(ctx)
    subs = []
    for s in range(40):
        inputs, want = case(R.LAYER2, 2, 6, seed=s % 3)
        subs.append((submit(b, R.LAYER2, inputs), want))
    for (t, got), want in subs:
        b.collect(t)
        assert bit_equal(got[0], want[0]) and bit_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    st = b.stats()
    b.close()
    return st


def check_hostile_ticket(ctx):
    b = Batcher(ctx)
    for layer in (R.LAYER1, R.LAYER2):
        failed = b.stats()["failed_tickets"]
        clean = [case(layer, nch, 2 if layer == R.LAYER1 else 1, seed=5 + nch) for nch in (1, 2, 2)]
        codes, rec, vvec, vfront = clean[1][0]
        bad_rec = rec.copy()
        bad_rec[1, 0, 7 if layer == R.LAYER1 else 32 + 7] = 1 if layer == R.LAYER1 else 64
        subs = [submit(b, layer, clean[0][0]), submit(b, layer, (codes, bad_rec, vvec, vfront)), submit(b, layer, clean[2][0])]
        b.collect(subs[0][0])
        with pytest.raises(SymaccelError) as e:
            b.collect(subs[1][0])
        assert e.value.status == _ffi.ERR_INVALID_ARG
        b.collect(subs[2][0])
        for i in (0, 2):
            assert bit_equal(subs[i][1][0], clean[i][1][0]) and bit_equal(subs[i][1][1], clean[i][1][1])
        assert b.stats()["failed_tickets"] == failed + 1
        # the batcher reads the records on the host (csrc/batcher.cpp check_mpa12): it must say what the kernel's status bytes say
        status = Mpa12Decode(ctx, layer).decode(codes, bad_rec, vvec, vfront)[3]
        assert status.sum() == 1 and status[1, 0] == 1
    b.close()


def check_formats(ctx):
    b = Batcher(ctx)
    for layer, nch, npk, fmt, dtype in ((R.LAYER1, 2, 9, "s16", np.int16), (R.LAYER2, 2, 6, "f32", np.float32), (R.LAYER2, 1, 1, "s16", np.int16)):
        inputs, want = case(layer, nch, npk)
        frames = npk * 32 * R.N_FRAMES[layer]
        t, slot = b.reserve(BATCH_MPA12_DECODE, layer, nch, npk, out_format=fmt, channels=nch)
        assert slot.input_bytes[0] == inputs[0].nbytes and slot.input_bytes[1] == inputs[1].nbytes and slot.state_bytes[0] == 4096 * nch
        assert slot.out_bytes == frames * nch * np.dtype(dtype).itemsize
        for ptr, a in ((slot.input[0], inputs[0]), (slot.input[1], inputs[1]), (slot.state[0], inputs[2]), (slot.state[1], inputs[3])):
            C.memmove(ptr, np.ascontiguousarray(a).ctypes.data, a.nbytes)
        b.commit(t)
        slot = b.wait(t)
        got = np.frombuffer((C.c_char * slot.out_bytes).from_address(slot.out), np.uint8).copy()
        vv = np.frombuffer((C.c_char * slot.state_bytes[0]).from_address(slot.state[0]), np.float32).reshape(nch, 1024).copy()
        b.release(t)
        native = want[0].reshape(nch, frames)
        assert np.array_equal(got, pcm_convert(ctx, native, fmt, channels=nch).ravel()), (layer, fmt)
        assert bit_equal(vv, want[1])
        if fmt == "f32":  # interleaving alone: the samples are the native ones
            assert bit_equal(got.view(np.float32).reshape(frames, nch).T, native)
    b.close()


def check_reserve_arguments(lib):
    ins, sts, out = (C.c_size_t * 6)(), (C.c_size_t * 3)(), C.c_size_t()
    assert lib.dll.symaccel_batcher_plane_bytes(BATCH_MPA12_DECODE, R.LAYER1, 5, ins, sts, C.byref(out)) == 0
    assert list(ins)[:3] == [5 * 768, 5 * 64, 0] and list(sts) == [4096, 4, 0] and out.value == 5 * 1536
    assert lib.dll.symaccel_batcher_plane_bytes(BATCH_MPA12_DECODE, R.LAYER2, 3, ins, sts, C.byref(out)) == 0
    assert list(ins)[:3] == [3 * 2304, 3 * 128, 0] and out.value == 3 * 4608
    for layer in (0, 3, -1):
        assert lib.dll.symaccel_batcher_plane_bytes(BATCH_MPA12_DECODE, layer, 3, ins, sts, C.byref(out)) == _ffi.ERR_INVALID_ARG


def test_kind_and_plane_sizes():
    assert BATCH_MPA12_DECODE == 10
    check_reserve_arguments(emu_library())


def test_emu_sharing(emu_ctx):
    check_sharing(emu_ctx)


def test_emu_many_chunks(emu_ctx, monkeypatch):
    monkeypatch.setenv("SYMACCEL_BATCH_CHUNK_MIN_KB", "64")
    monkeypatch.setenv("SYMACCEL_BATCH_CHUNKS", "64")
    st = check_many_chunks(emu_ctx)
    assert (st["launches"], st["chunks"]) == (1, 20), st


def test_emu_default_chunking_is_one_chunk(emu_ctx, monkeypatch):
    monkeypatch.delenv("SYMACCEL_BATCH_CHUNK_MIN_KB", raising=False)
    monkeypatch.delenv("SYMACCEL_BATCH_CHUNKS", raising=False)
    st = check_many_chunks(emu_ctx)
    assert (st["launches"], st["chunks"]) == (1, 1), st


def test_emu_hostile_ticket(emu_ctx):
    check_hostile_ticket(emu_ctx)


def test_emu_formats(emu_ctx):
    check_formats(emu_ctx)


@pytest.mark.gpu
def test_gpu_sharing(gpu_ctx):
    check_sharing(gpu_ctx)


@pytest.mark.gpu
def test_gpu_many_chunks(gpu_ctx, monkeypatch):
    monkeypatch.setenv("SYMACCEL_BATCH_CHUNK_MIN_KB", "64")
    monkeypatch.setenv("SYMACCEL_BATCH_CHUNKS", "64")
    st = check_many_chunks(gpu_ctx)
    assert (st["launches"], st["chunks"]) == (1, 20), st


@pytest.mark.gpu
def test_gpu_hostile_ticket(gpu_ctx):
    check_hostile_ticket(gpu_ctx)


@pytest.mark.gpu
def test_gpu_formats(gpu_ctx):
    check_formats(gpu_ctx)
