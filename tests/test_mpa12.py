"""MPEG Layer I / Layer II from sample codes (symaccel_mpa12_decode*, the fused form of mpa_polyphase_kernel): dequantisation, scaling and
the polyphase filterbank in one kernel, against tests/mpa12_ref.py (the reference's arithmetic in numpy float32, pinned here to what the
interpreted reference decoded: tests/golden/mpa12) + the oracle's polyphase -- bit for bit: PCM, v_vec, v_front, status.  In CPU emulation
and, gpu-marked, on the MI355X."""
import functools
import json

import numpy as np
import pytest

import mpa12_ref as R
from emu_lib import emu_ctx, emu_library  # noqa: F401
from helpers import bit_equal
from test_pingpong import HostTensor

L1_SHAPES = [(nch, npk, 2) for nch in (1, 2, 3) for npk in (1, 2, 9)]   # a segment (2) as long as the halo, shorter than the chain
L2_SHAPES = [(nch, npk, 1) for nch in (1, 2, 3) for npk in (1, 6)]
SHAPES = [(R.LAYER1,) + s for s in L1_SHAPES] + [(R.LAYER2,) + s for s in L2_SHAPES]


def width_of(layer, alloc):
    return alloc if layer == R.LAYER1 else int(R.tables()["width"][alloc - 1])


@functools.lru_cache(maxsize=None)
def case(layer, nch, npk, seed=0):
    """(codes, rec, vvec, vfront) and what the reference makes of them.  Every channel-packet: every bit width / class on some
    sub-band and unallocated ones; per allocated sub-band the codes 0, 2^w - 1, 2^(w-1), the one that makes a + 1 == 0 and random
    16-bit ones (bits above the width set: they are masked); scale-factor indices over 0..63 with 63 present; a random state."""
    rng = np.random.default_rng(1000 * layer + 100 * nch + npk + seed)
    nf, rb = R.N_FRAMES[layer], R.RECORD_BYTES[layer]
    allowed = np.array([0] + (list(range(2, 16)) if layer == R.LAYER1 else list(range(1, 18))))
    codes = rng.integers(0, 1 << 16, (nch, npk, 32, nf)).astype(np.uint16)
    rec = np.zeros((nch, npk, rb), np.uint8)
    for c in range(nch):
        for p in range(npk):
            alloc = rng.permutation(np.concatenate([allowed, rng.choice(allowed, 32 - len(allowed))]))
            rec[c, p, :32] = alloc
            rec[c, p, 32:] = rng.integers(0, 64, rb - 32)
            rec[c, p, 32 + int(rng.integers(0, rb - 32))] = 63
            for sb in range(32):
                if alloc[sb]:
                    w = width_of(layer, int(alloc[sb]))
                    special = np.array([0, (1 << w) - 1, 1 << (w - 1), (1 << (w - 1)) - 1], np.uint16)
                    at = rng.choice(nf, 4, replace=False)
                    codes[c, p, sb, at] = special | (codes[c, p, sb, at] & np.uint16((0xffff << w) & 0xffff) if (c + p) % 2 else np.uint16(0))
    vvec = rng.standard_normal((nch, 1024)).astype(np.float32)
    vfront = rng.integers(0, 16, nch).astype(np.int32)
    want = R.decode(layer, codes, rec, vvec, vfront)
    for a in (codes, rec, vvec, vfront) + want:
        a.setflags(write=False)
    return (codes, rec, vvec, vfront), want


def check(got, want, what):
    pcm, vv, vf, st = got
    assert bit_equal(pcm, want[0]), what + ": pcm"
    assert bit_equal(vv, want[1]), what + ": v_vec"
    assert np.array_equal(vf, want[2]), what + ": v_front"
    assert np.array_equal(st, want[3]), what + ": status"


def run_device(ctx, wrap, unwrap, layer, inputs, want, seg):
    """the ping-pong entry point, the in-place one and the unfused kernel fed the reference's dequantised samples"""
    from symphonia_amd import Mpa12Decode, MpaPolyphase
    codes, rec, vvec, vfront = inputs
    nch, npk = codes.shape[:2]
    dec = Mpa12Decode(ctx, layer)
    assert dec.record_bytes == R.RECORD_BYTES[layer]
    ctx.set_segment(seg)
    try:
        d_codes, d_rec = wrap(codes), wrap(rec)
        pcm, st = wrap(np.full((nch, npk, 32 * dec.n_frames), np.nan, np.float32)), wrap(np.full((nch, npk), 7, np.uint8))
        vv_in, vf_in = wrap(vvec.copy()), wrap(vfront.copy())
        vv_out, vf_out = wrap(np.full((nch, 1024), np.nan, np.float32)), wrap(np.full(nch, -1, np.int32))
        dec.decode(d_codes, d_rec, vv_in, vf_in, pcm=pcm, state_out=(vv_out, vf_out), status=st)
        check((unwrap(pcm), unwrap(vv_out), unwrap(vf_out), unwrap(st)), want, "pp_device")
        assert bit_equal(unwrap(vv_in), vvec) and np.array_equal(unwrap(vf_in), vfront), "the incoming state is read only"
        pcm2, st2 = wrap(np.full((nch, npk, 32 * dec.n_frames), np.nan, np.float32)), wrap(np.full((nch, npk), 7, np.uint8))
        dec.decode(d_codes, d_rec, vv_in, vf_in, pcm=pcm2, status=st2)
        check((unwrap(pcm2), unwrap(vv_in), unwrap(vf_in), unwrap(st2)), want, "device")
        # fused == unfused: the old kernel on the f32 sub-band samples the reference's dequantisation gives
        x = R.dequantize_batch(layer, codes, rec)
        vv3, vf3 = wrap(vvec.copy()), wrap(vfront.copy())
        pcm3 = wrap(np.full(x.shape, np.nan, np.float32))
        MpaPolyphase(ctx, dec.n_frames).synth(wrap(x), vv3, vf3, pcm3)
        assert bit_equal(unwrap(pcm3), unwrap(pcm)) and bit_equal(unwrap(vv3), unwrap(vv_out)) and np.array_equal(unwrap(vf3), unwrap(vf_out)), "unfused"
    finally:
        ctx.set_segment(0)


def run_host(ctx, layer, inputs, want, seg):
    from symphonia_amd import Mpa12Decode
    ctx.set_segment(seg)
    try:
        check(Mpa12Decode(ctx, layer).decode(*inputs), want, "host form")
    finally:
        ctx.set_segment(0)


def hostile_case(layer):
    """3 chains x 5 packets; chain 1 carries one out-of-range record per kind in packets 1..3 (packets 0 and 4 and the other chains
    are clean)"""
    (codes, rec, vvec, vfront), _ = case(layer, 3, 5, seed=77)
    rec = rec.copy()
    if layer == R.LAYER1:
        rec[1, 1, 5], rec[1, 2, 31], rec[1, 3, 32 + 9] = 1, 16, 64          # bits of 1, bits above 15, a scale factor above 63
        rec[2, 4, 0], rec[2, 4, 63] = 255, 255
    else:
        rec[1, 1, 5], rec[1, 2, 31], rec[1, 3, 96 + 9] = 18, 255, 64        # classes above 17, a scale factor above 63 (third part)
        rec[2, 4, 0], rec[2, 4, 32] = 200, 255
    return (codes, rec, vvec, vfront)


def run_hostile(decode_fn, layer):
    inputs = hostile_case(layer)
    want = R.decode(layer, *inputs)
    assert want[3].sum() == 4 and want[3][1, 1:4].all() and want[3][2, 4] == 1
    got = decode_fn(inputs)
    check(got, want, "hostile")
    # the same as a stream whose marked packets allocate nothing: silence for those packets alone, the filterbank advances
    clean = inputs[1].copy()
    clean[want[3] == 1] = 0
    again = decode_fn((inputs[0], clean) + inputs[2:])
    assert not again[3].any()
    assert bit_equal(again[0], got[0]) and bit_equal(again[1], got[1]) and np.array_equal(again[2], got[2])


# ---- CPU: the reference file, the tables, the emulation build

def fixture_streams():
    s = np.load(R.GOLDEN / "streams.npz")
    return s, json.loads(bytes(s["manifest"]).decode())["entries"]


def test_ref_is_the_reference():
    """mpa12_ref + oracle on the codes and records the writer put into the fixture packets == what Layer1::decode / Layer2::decode
    made of the packets under the interpreter, and the streams cover what the formats allow"""
    s, entries = fixture_streams()
    seen_bits, seen_class, bounds, tables_, crc = set(), set(), {1: set(), 2: set()}, set(), set()
    for e in entries:
        n, layer = e["name"], e["layer"]
        codes, rec = s[n + "_codes"], s[n + "_rec"]
        nch = codes.shape[0]
        pcm, vv, vf, st = R.decode(layer, codes, rec, np.zeros((nch, 1024), np.float32), np.zeros(nch, np.int32))
        assert not st.any()
        assert np.array_equal(pcm.view(np.uint32), s[n + "_pcm"]), n
        assert np.array_equal(vv.view(np.uint32), s[n + "_vvec"]) and np.array_equal(vf, s[n + "_vfront"]), n
        (seen_bits if layer == 1 else seen_class).update(int(x) for x in np.unique(rec[..., :32]))
        bounds[layer].add(e["bound"] if e["mode"] == 1 else None)
        tables_.add(e["alloc_table"])
        crc.add((layer, e["crc"]))
        if layer == 2:
            assert (rec[..., 32:] == 63).any()
    assert seen_bits == set([0] + list(range(2, 16))) and seen_class == set(range(18))
    assert bounds[1] >= {4, 8, 12, 16, None} and bounds[2] >= {4, 8, 12, 16, None}
    assert tables_ >= {"a", "b", "c", "d", "m2"} and crc == {(1, False), (1, True), (2, False), (2, True)}


def test_host_tables_are_the_reference_bits():
    from symphonia_amd import _ffi
    got = emu_library().table(_ffi.TABLE_MPA12)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), R.packed_tables().view(np.uint32))
    assert len(emu_library().table(_ffi.TABLE_MP3_CONSTS)) == 264


def test_record_bytes():
    d = emu_library().dll
    assert [d.symaccel_mpa12_record_bytes(k) for k in (0, 1, 2, 3)] == [0, 64, 128, 0]


@pytest.mark.parametrize("layer,nch,npk,seg", SHAPES)
def test_emu_mpa12_device(emu_ctx, layer, nch, npk, seg):
    inputs, want = case(layer, nch, npk)
    run_device(emu_ctx, HostTensor, lambda t: t.a, layer, inputs, want, seg)


@pytest.mark.parametrize("layer,nch,npk,seg", SHAPES)
def test_emu_mpa12_host(emu_ctx, layer, nch, npk, seg):
    inputs, want = case(layer, nch, npk)
    run_host(emu_ctx, layer, inputs, want, seg)


def run_no_packets(ctx, wrap, unwrap, layer):
    """0 packets: nothing is launched -- through `_pp_device`, the in-place device form and the host form the incoming state, the
    outgoing state buffers, the PCM and the status planes are all left as they were"""
    from symphonia_amd import Mpa12Decode
    rng = np.random.default_rng(3)
    nf, rb = R.N_FRAMES[layer], R.RECORD_BYTES[layer]
    vv, vf = rng.standard_normal((2, 1024)).astype(np.float32), np.array([3, 9], np.int32)
    codes, rec = np.zeros((2, 0, 32, nf), np.uint16), np.zeros((2, 0, rb), np.uint8)
    dec = Mpa12Decode(ctx, layer)
    d_vv, d_vf = wrap(vv.copy()), wrap(vf.copy())
    out_vv, out_vf = wrap(np.full((2, 1024), 5.0, np.float32)), wrap(np.full(2, -1, np.int32))
    pcm, st = wrap(np.full((2, 1, 32 * nf), 7.0, np.float32)), wrap(np.full((2, 1), 7, np.uint8))  # (room for a packet nobody may write)
    dec.decode(wrap(codes), wrap(rec), d_vv, d_vf, pcm=pcm, state_out=(out_vv, out_vf), status=st)
    dec.decode(wrap(codes), wrap(rec), d_vv, d_vf, pcm=pcm, status=st)
    ctx.sync()
    assert bit_equal(unwrap(d_vv), vv) and np.array_equal(unwrap(d_vf), vf), "the incoming state"
    assert np.all(unwrap(out_vv) == 5.0) and np.all(unwrap(out_vf) == -1), "the outgoing state buffers"
    assert np.all(unwrap(pcm) == 7.0) and np.all(unwrap(st) == 7), "PCM and status"
    got = dec.decode(codes, rec, vv, vf)
    assert got[0].shape == (2, 0, 32 * nf) and bit_equal(got[1], vv) and np.array_equal(got[2], vf) and got[3].shape == (2, 0)


@pytest.mark.parametrize("layer", [R.LAYER1, R.LAYER2])
def test_emu_mpa12_no_packets(emu_ctx, layer):
    run_no_packets(emu_ctx, HostTensor, lambda t: t.a, layer)


@pytest.mark.parametrize("layer", [R.LAYER1, R.LAYER2])
def test_emu_mpa12_hostile_records(emu_ctx, layer):
    from symphonia_amd import Mpa12Decode
    run_hostile(lambda inputs: Mpa12Decode(emu_ctx, layer).decode(*inputs), layer)


def test_emu_mpa12_fixture_streams(emu_ctx):
    """the packets' codes and records through the library == the PCM the interpreted reference decoded the packets to"""
    from symphonia_amd import Mpa12Decode
    s, entries = fixture_streams()
    for e in entries:
        n = e["name"]
        nch = e["channels"]
        got = Mpa12Decode(emu_ctx, e["layer"]).decode(s[n + "_codes"], s[n + "_rec"], np.zeros((nch, 1024), np.float32), np.zeros(nch, np.int32))
        assert np.array_equal(got[0].view(np.uint32), s[n + "_pcm"]) and np.array_equal(got[1].view(np.uint32), s[n + "_vvec"]), n
        assert np.array_equal(got[2], s[n + "_vfront"]) and not got[3].any(), n


def test_argument_errors(emu_ctx):
    """reported before anything is launched: the outputs stay as they were"""
    import ctypes as C
    from symphonia_amd import _ffi
    d, h = emu_ctx.lib.dll, emu_ctx.handle
    codes, rec = np.zeros((1, 1, 32, 12), np.uint16), np.zeros((1, 1, 64), np.uint8)
    vv, vv2, vf, vf2 = np.zeros(1024, np.float32), np.zeros(1024, np.float32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    pcm, st = np.full(384, np.nan, np.float32), np.full(1, 7, np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    pp, io, host = d.symaccel_mpa12_decode_pp_device, d.symaccel_mpa12_decode_device, d.symaccel_mpa12_decode
    assert pp(h, 3, p(codes), p(rec), p(vv), p(vf), p(vv2), p(vf2), p(pcm), p(st), 1, 1) == _ffi.ERR_UNSUPPORTED
    assert io(h, 0, p(codes), p(rec), p(vv), p(vf), p(pcm), p(st), 1, 1) == _ffi.ERR_UNSUPPORTED
    assert host(h, 3, p(codes), p(rec), p(vv), p(vf), p(pcm), p(st), 1, 1) == _ffi.ERR_UNSUPPORTED
    assert pp(None, 1, p(codes), p(rec), p(vv), p(vf), p(vv2), p(vf2), p(pcm), p(st), 1, 1) == _ffi.ERR_INVALID_ARG
    assert pp(h, 1, p(codes), p(rec), p(vv), p(vf), p(vv), p(vf2), p(pcm), p(st), 1, 1) == _ffi.ERR_INVALID_ARG   # aliased v_vec
    assert pp(h, 1, p(codes), p(rec), p(vv), p(vf), p(vv2), p(vf), p(pcm), p(st), 1, 1) == _ffi.ERR_INVALID_ARG   # aliased v_front
    assert pp(h, 1, None, p(rec), p(vv), p(vf), p(vv2), p(vf2), p(pcm), p(st), 1, 1) == _ffi.ERR_INVALID_ARG
    assert pp(h, 2, p(codes), None, p(vv), p(vf), p(vv2), p(vf2), p(pcm), p(st), 1, 1) == _ffi.ERR_INVALID_ARG
    assert pp(h, 1, C.c_void_p(p(codes) + 2), p(rec), p(vv), p(vf), p(vv2), p(vf2), p(pcm), p(st), 1, 1) == _ffi.ERR_INVALID_ARG  # codes not 8-byte aligned
    assert io(h, 1, p(codes), p(rec), None, p(vf), p(pcm), p(st), 1, 1) == _ffi.ERR_INVALID_ARG
    assert host(h, 1, p(codes), p(rec), p(vv), p(vf), None, p(st), 1, 1) == _ffi.ERR_INVALID_ARG
    assert pp(h, 1, p(codes), p(rec), p(vv), p(vf), p(vv2), p(vf2), p(pcm), None, 1, 1) == _ffi.OK   # the status plane is optional
    emu_ctx.sync()
    assert st[0] == 7


# ---- GPU

def gpu_wrap(a):
    import torch
    a = np.array(a, order="C")  # (a copy: the shared cases are read-only)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def gpu_unwrap(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def gpu_ctx():
    import torch
    from symphonia_amd import Context
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    with Context(0) as ctx:
        ctx.use_torch_stream()
        yield ctx


@pytest.mark.gpu
@pytest.mark.parametrize("layer,nch,npk,seg", SHAPES + [(R.LAYER1, 9, 40, 0), (R.LAYER1, 9, 40, 5), (R.LAYER2, 9, 33, 0), (R.LAYER2, 9, 33, 3)])
def test_gpu_mpa12_device(gpu_ctx, layer, nch, npk, seg):
    inputs, want = case(layer, nch, npk)
    run_device(gpu_ctx, gpu_wrap, gpu_unwrap, layer, inputs, want, seg)


@pytest.mark.gpu
@pytest.mark.parametrize("layer,nch,npk,seg", SHAPES)
def test_gpu_mpa12_host(gpu_ctx, layer, nch, npk, seg):
    inputs, want = case(layer, nch, npk)
    run_host(gpu_ctx, layer, inputs, want, seg)


@pytest.mark.gpu
@pytest.mark.parametrize("layer", [R.LAYER1, R.LAYER2])
def test_gpu_mpa12_no_packets(gpu_ctx, layer):
    run_no_packets(gpu_ctx, gpu_wrap, gpu_unwrap, layer)


@pytest.mark.gpu
@pytest.mark.parametrize("layer", [R.LAYER1, R.LAYER2])
def test_gpu_mpa12_hostile_records(gpu_ctx, layer):
    from symphonia_amd import Mpa12Decode
    run_hostile(lambda inputs: Mpa12Decode(gpu_ctx, layer).decode(*inputs), layer)


@pytest.mark.gpu
def test_gpu_mpa12_fixture_streams(gpu_ctx):
    """the frozen runs of the interpreted reference, replayed on the device (reads tests/golden/mpa12 only)"""
    from symphonia_amd import Mpa12Decode
    s, entries = fixture_streams()
    for e in entries:
        n, nch = e["name"], e["channels"]
        got = Mpa12Decode(gpu_ctx, e["layer"]).decode(s[n + "_codes"], s[n + "_rec"], np.zeros((nch, 1024), np.float32), np.zeros(nch, np.int32))
        assert np.array_equal(got[0].view(np.uint32), s[n + "_pcm"]) and np.array_equal(got[1].view(np.uint32), s[n + "_vvec"]), n
        assert np.array_equal(got[2], s[n + "_vfront"]) and not got[3].any(), n
