"""The batcher's eleventh kind, SYMACCEL_BATCH_PCM_DECODE: a chain is one packet, units_per_chain its frames, param = codec | channels << 8 |
shift << 16 (symphonia-codec-pcm lib.rs:318-411: no state passes from packet to packet, no packet can fail).  Packets of many streams
share the launch of their (codec, channels, shift, frames); every result equals the direct call symaccel_pcm_decode and the numpy
restatement (tests/pcm_decode_ref.py, pinned to the reference fixture by tests/test_pcm_decode.py); an output format is delivered by the
decode kernel itself, a packet's channels being the interleave group, so formats split launches; a param the direct call refuses fails at reserve(); a
packet of zero frames is a submission like any other and comes back empty.  CPU emulation here, gpu-marked twins on the MI355X."""
import ctypes as C

import numpy as np
import pytest

from emu_lib import emu_ctx, emu_library  # noqa: F401
from symphonia_amd import BATCH_PCM_DECODE, Batcher, Context, SymaccelError, pcm_decode
from symphonia_amd import _ffi
from test_pcm_convert import BYTES, FMT

import pcm_decode_ref as R

# codec, channels, shift, frames
SHAPES = [("s16le", 2, 0, 100), ("s24be", 2, 4, 100), ("mulaw", 1, 0, 160), ("f32le", 8, 0, 33), ("s24le", 3, 0, 77), ("f64be", 1, 0, 100), ("u8", 2, 7, 100)]


def param(codec, ch, shift=0):
    return (R.NAMES.index(codec) + 1) | ch << 8 | shift << 16


def packets(rng, codec, ch, frames, n):
    return rng.integers(0, 256, (n, frames * ch * R.coded_bytes(codec)), dtype=np.uint8)


@pytest.fixture(scope="module")
def gpu_ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on an MI355X (there is no CPU path)")
    ctx = Context(0)
    yield ctx
    ctx.close()


def check_sharing(ctx):
    rng = np.random.default_rng(61)
    b = Batcher(ctx)
    subs = []
    for s in range(28):  # twenty-eight streams, seven shapes, submissions of one to five packets
        codec, ch, shift, frames = SHAPES[s % len(SHAPES)]
        p = packets(rng, codec, ch, frames, 1 + s % 5)
        out = np.zeros((len(p), ch, frames), R.NATIVE_DTYPE[R.CODECS[codec][3]])
        subs.append((b.submit_pcm_decode(p, codec, ch, out, shift=shift), p, codec, ch, shift, frames, out))
    assert b.stats()["pending"] == 28
    for t, p, codec, ch, shift, frames, out in subs:
        b.collect(t)
        want = R.decode(p, codec, ch, frames, shift)
        assert np.array_equal(out.view(np.uint8), want.view(np.uint8)), (codec, ch)
        direct = pcm_decode(ctx, p, codec, ch, frames, shift)
        assert direct.dtype == out.dtype and np.array_equal(out.view(np.uint8), direct.view(np.uint8)), (codec, ch)
    st = b.stats()
    assert st["launches"] == len(SHAPES) < st["submissions"] == 28 and st["failed_tickets"] == 0, st
    assert st["chains_launched"] == sum(1 + s % 5 for s in range(28))
    b.close()


def check_frame_counts_and_shifts_split(ctx):
    """the same codec at two frame counts and two shifts: four groups, four launches"""
    rng = np.random.default_rng(67)
    b = Batcher(ctx)
    subs = []
    for frames, shift in ((50, 0), (51, 0), (50, 3), (51, 3), (50, 0), (51, 3)):
        p = packets(rng, "u16be", 2, frames, 2)
        out = np.zeros((2, 2, frames), np.uint16)
        subs.append((b.submit_pcm_decode(p, "u16be", 2, out, shift=shift), p, frames, shift, out))
    for t, p, frames, shift, out in subs:
        b.collect(t)
        assert np.array_equal(out, R.decode(p, "u16be", 2, frames, shift))
    st = b.stats()
    assert st["launches"] == 4 and st["submissions"] == 6 and st["chains_launched"] == 12, st
    b.close()


def check_zero_frame_packets(ctx):
    """a packet of zero frames (an empty packet, or one shorter than a frame: lib.rs:320) is a submission like any other: a ticket, empty
    planes, nothing written, no failure -- natively, with a format and through the zero-copy form; its neighbours decode as ever"""
    rng = np.random.default_rng(73)
    b = Batcher(ctx)
    p1 = packets(rng, "s16le", 2, 10, 2)
    o1 = np.zeros((2, 2, 10), np.int16)
    t1 = b.submit_pcm_decode(p1, "s16le", 2, o1)
    o0 = np.zeros((3, 2, 0), np.int16)
    t0 = b.submit_pcm_decode(np.zeros((3, 0), np.uint8), "s16le", 2, o0)
    guard = np.full(64, 0xA5, np.uint8)
    t0f = b.submit_pcm_decode(np.zeros((1, 0), np.uint8), "s24be", 3, guard[:0].reshape(1, 0), out_format="f32")
    p2 = packets(rng, "s16le", 2, 10, 1)
    o2 = np.zeros((1, 2, 10), np.int16)
    t2 = b.submit_pcm_decode(p2, "s16le", 2, o2)
    for t in (t0, t2, t0f, t1):
        b.collect(t)
    assert np.array_equal(o1, R.decode(p1, "s16le", 2, 10)) and np.array_equal(o2, R.decode(p2, "s16le", 2, 10)) and np.all(guard == 0xA5)
    t, slot = b.reserve(BATCH_PCM_DECODE, param("f64le", 8), 4, 0)
    assert slot.input_bytes[0] == 0 and slot.out_bytes == 0
    b.commit(t)
    assert b.wait(t).out_bytes == 0
    b.release(t)
    st = b.stats()
    assert st["submissions"] == 5 and st["failed_tickets"] == 0 and st["pending"] == 0, st
    b.close()
    assert pcm_decode(ctx, np.zeros((3, 0), np.uint8), "s16le", 2).shape == (3, 2, 0)  # the per-stream call: the same nothing


def check_formats(ctx):
    rng = np.random.default_rng(71)
    b = Batcher(ctx)
    subs = []
    for k, fmt in enumerate(FMT):
        codec, ch, shift, frames = SHAPES[k % 4]
        p = packets(rng, codec, ch, frames, 2 + k % 3)
        out = np.zeros((len(p), frames * ch * BYTES[fmt]), np.uint8)
        subs.append((b.submit_pcm_decode(p, codec, ch, out, shift=shift, out_format=fmt), p, codec, ch, shift, frames, out, fmt))
    # two submissions of one shape and one format share a launch; the same shape in another format does not
    codec, ch, shift, frames = SHAPES[0]
    twins = []
    for fmt in ("f32", "f32", "u8"):
        p = packets(rng, codec, ch, frames, 3)
        out = np.zeros((3, frames * ch * BYTES[fmt]), np.uint8)
        twins.append((b.submit_pcm_decode(p, codec, ch, out, shift=shift, out_format=fmt), p, codec, ch, shift, frames, out, fmt))
    for t, p, codec, ch, shift, frames, out, fmt in subs + twins:
        b.collect(t)
        assert np.array_equal(out, R.interleave(R.decode(p, codec, ch, frames, shift), R.CODECS[codec][3], fmt)), (codec, fmt)
    st = b.stats()
    # nine formats over four shapes: nine groups; the twins: f32 of shape 0 is the group of k = 8 (f32, shape 0), u8 of shape 0 that of k = 0
    assert st["submissions"] == 12 and st["launches"] == 9 and st["failed_tickets"] == 0, st
    # the zero-copy form: out_bytes is the converted size from reserve() on
    p = packets(rng, "s24be", 2, 35, 5)
    t, slot = b.reserve(BATCH_PCM_DECODE, param("s24be", 2), 5, 35, out_format="s16", channels=2)
    assert slot.input_bytes[0] == p.size and slot.out_bytes == 5 * 35 * 2 * 2
    np.ctypeslib.as_array((C.c_uint8 * p.size).from_address(slot.input[0]))[:] = p.ravel()
    b.commit(t)
    slot = b.wait(t)
    got = np.ctypeslib.as_array((C.c_uint8 * (5 * 35 * 2 * 2)).from_address(slot.out)).reshape(5, -1).copy()
    b.release(t)
    assert np.array_equal(got, R.interleave(R.decode(p, "s24be", 2, 35), "s24", "s16"))
    for bad in ((param("s24be", 2), 5, 35, "s16", 1), (param("s24be", 2), 5, 35, 10, 2), (param("s24be", 2) | 4 << 24, 5, 35, "s16", 2)):  # channels, format, a format inside param
        with pytest.raises(SymaccelError) as e:
            b.reserve(BATCH_PCM_DECODE, bad[0], bad[1], bad[2], out_format=bad[3], channels=bad[4])
        assert e.value.status == _ffi.ERR_INVALID_ARG
    b.close()


def check_reserve_refusals(ctx):
    b = Batcher(ctx)
    bad = [param("s16le", 0), param("s16le", 9), param("s16le", 2, 16), param("s16le", 2, 17), param("alaw", 1, 1), param("f32be", 2, 5), 0 | 2 << 8, 21 | 2 << 8,
           param("s16le", 2) | 1 << 24, -1]
    for p in bad:
        with pytest.raises(SymaccelError) as e:
            b.reserve(BATCH_PCM_DECODE, p, 2, 64)
        assert e.value.status == _ffi.ERR_INVALID_ARG, p
    with pytest.raises(SymaccelError) as e:  # zero frames are a packet only for this kind
        b.reserve(9, 3 | 2 << 8, 2, 0)
    assert e.value.status == _ffi.ERR_INVALID_ARG
    for p in (param("s16le", 9), param("alaw", 1, 1)):  # ... and a bad param stays bad at zero frames
        with pytest.raises(SymaccelError):
            b.reserve(BATCH_PCM_DECODE, p, 2, 0)
    t, slot = b.reserve(BATCH_PCM_DECODE, param("s24le", 3, 23), 3, 1)  # one frame, the largest shift
    assert slot.input_bytes[0] == 3 * 9 and slot.out_bytes == 3 * 3 * 4
    b.release(t)
    assert b.stats()["failed_tickets"] == 0
    b.close()


def test_streams_of_mixed_codecs_share_launches(emu_ctx):  # noqa: F811
    check_sharing(emu_ctx)


def test_frame_counts_and_shifts_go_to_launches_of_their_own(emu_ctx):  # noqa: F811
    check_frame_counts_and_shifts_split(emu_ctx)


def test_output_formats_through_the_batcher(emu_ctx):  # noqa: F811
    check_formats(emu_ctx)


def test_zero_frame_packets(emu_ctx):  # noqa: F811
    check_zero_frame_packets(emu_ctx)


def test_bad_params_fail_at_reserve(emu_ctx):  # noqa: F811
    check_reserve_refusals(emu_ctx)


def test_kind_value_and_plane_bytes():
    assert BATCH_PCM_DECODE == 11
    lib = emu_library()
    ins, sts, out = (C.c_size_t * 6)(), (C.c_size_t * 3)(), C.c_size_t()
    assert lib.dll.symaccel_batcher_plane_bytes(BATCH_PCM_DECODE, param("s24be", 2, 4), 1000, ins, sts, C.byref(out)) == 0
    assert list(ins) == [6000, 0, 0, 0, 0, 0] and list(sts) == [0, 0, 0] and out.value == 2 * 1000 * 4
    assert lib.dll.symaccel_batcher_plane_bytes(BATCH_PCM_DECODE, param("mulaw", 1), 160, ins, sts, C.byref(out)) == 0 and (ins[0], out.value) == (160, 320)
    assert lib.dll.symaccel_batcher_plane_bytes(BATCH_PCM_DECODE, param("f64le", 8), 7, ins, sts, C.byref(out)) == 0 and (ins[0], out.value) == (448, 448)
    assert lib.dll.symaccel_batcher_plane_bytes(BATCH_PCM_DECODE, param("mulaw", 1, 2), 160, ins, sts, C.byref(out)) == _ffi.ERR_INVALID_ARG
    assert lib.dll.symaccel_batcher_plane_bytes(BATCH_PCM_DECODE, param("s16le", 9), 160, ins, sts, C.byref(out)) == _ffi.ERR_INVALID_ARG


@pytest.mark.gpu
def test_gpu_streams_of_mixed_codecs_share_launches(gpu_ctx):
    check_sharing(gpu_ctx)


@pytest.mark.gpu
def test_gpu_frame_counts_and_shifts_go_to_launches_of_their_own(gpu_ctx):
    check_frame_counts_and_shifts_split(gpu_ctx)


@pytest.mark.gpu
def test_gpu_output_formats_through_the_batcher(gpu_ctx):
    check_formats(gpu_ctx)


@pytest.mark.gpu
def test_gpu_zero_frame_packets(gpu_ctx):
    check_zero_frame_packets(gpu_ctx)


@pytest.mark.gpu
def test_gpu_bad_params_fail_at_reserve(gpu_ctx):
    check_reserve_refusals(gpu_ctx)
