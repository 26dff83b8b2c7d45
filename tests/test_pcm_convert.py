"""PCM in the caller's sample format: symaccel_pcm_convert(_device) against the reference's FromSample conversions
(symphonia-core/src/audio/conv.rs:521-532 from i32, 596-607 from f32) and the interleave of audio/util.rs:119-167.

Expected bytes come from two independent places that must agree:
  * tests/golden/pcm_convert.npz -- the reference's conv.rs executed under tools/rsinterp (tools/make_pcm_fixtures.py; the localref case
    below regenerates it from the reference tree and compares);
  * `restate()` -- a plain numpy restatement of the conversion contract, written from the contract and not from the kernel.
The restatement is checked against the fixture on every fixture input; the kernel is checked against the fixture there and against the
restatement on the full sweeps (every 16-bit step k / 32768 with both neighbouring floats, a few hundred 24-bit steps, the special values;
for i32 the extremes and every power of two +- 1).  Every comparison is on bytes, no tolerance.  CPU emulation here, gpu-marked twins on
the MI355X."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from emu_lib import emu_ctx, emu_library  # noqa: F401
from symphonia_amd import (FMT_F32, FMT_S8, FMT_S16, FMT_S24, FMT_S32, FMT_U8, FMT_U16, FMT_U24, FMT_U32, Context, SymaccelError, pcm_convert,
                           pcm_convert_device, sample_bytes)

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_pcm_fixtures as M  # noqa: E402  (the inputs of the sweeps: the fixture's generators at full density)

GOLDEN = ROOT / "tests" / "golden" / "pcm_convert.npz"
FMT = {"u8": FMT_U8, "s8": FMT_S8, "u16": FMT_U16, "s16": FMT_S16, "u24": FMT_U24, "s24": FMT_S24, "u32": FMT_U32, "s32": FMT_S32, "f32": FMT_F32}
BYTES = {"u8": 1, "s8": 1, "u16": 2, "s16": 2, "u24": 3, "s24": 3, "u32": 4, "s32": 4, "f32": 4}
BITS = {"u8": 8, "s8": 8, "u16": 16, "s16": 16, "u24": 24, "s24": 24, "u32": 32, "s32": 32}
DESTS = tuple(FMT)
PAIRS = [(s, d) for s in ("f32", "s32") for d in DESTS]


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------

def _as_int(v, lo, hi):
    """Rust's `v as <integer>`: toward zero, saturating, NaN -> 0 (as int64)"""
    v = np.asarray(v)
    out = np.zeros(v.shape, np.int64)
    ok = ~np.isnan(v)
    t = np.trunc(np.clip(v[ok].astype(np.float64), float(lo), float(hi)))  # (every bound is exact in f64; f32 -> f64 is exact)
    out[ok] = t.astype(np.int64)
    return out


def _le_bytes(v, nbytes):
    """the low `nbytes` bytes of each value, little-endian: uint8[n, nbytes]"""
    return (np.asarray(v, np.int64) & 0xffffffff).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :nbytes].copy()


def restate(src, dst, x):
    """x: float32 (src 'f32') or int32 (src 's32') -> uint8[n, bytes of dst]"""
    if src == "f32":
        x = np.asarray(x, np.float32)
        if dst == "f32":
            return x.view(np.uint8).reshape(-1, 4).copy()
        with np.errstate(invalid="ignore", over="ignore"):
            c = np.where(x > np.float32(1.0), np.float32(1.0), x)  # clamp_f32: two comparisons, a NaN fails both
            c = np.where(c < np.float32(-1.0), np.float32(-1.0), c).astype(np.float32)
            n = BITS[dst]
            if dst[0] == "u":
                if n == 32:
                    v = (c + np.float32(1.0)).astype(np.float32).astype(np.float64) * 2147483648.0
                else:
                    v = ((c + np.float32(1.0)).astype(np.float32) * np.float32(2.0 ** (n - 1))).astype(np.float32)  # two rounded f32 operations
                if n == 24:
                    return _le_bytes(np.minimum(_as_int(v, 0, 2 ** 32 - 1), 0xffffff), 3)  # `as u32`, then u24::from clamps
                return _le_bytes(_as_int(v, 0, 2 ** n - 1), n // 8)
            v = c.astype(np.float64) * 2147483648.0 if n == 32 else (c * np.float32(2.0 ** (n - 1))).astype(np.float32)
            if n == 24:
                return _le_bytes(np.clip(_as_int(v, -2 ** 31, 2 ** 31 - 1), -2 ** 23, 2 ** 23 - 1), 3)  # `as i32`, then i24::from clamps
            return _le_bytes(_as_int(v, -2 ** (n - 1), 2 ** (n - 1) - 1), n // 8)
    s = np.asarray(x, np.int32).astype(np.int64)
    if dst == "f32":
        return (s.astype(np.float64) / 2147483648.0).astype(np.float32).view(np.uint8).reshape(-1, 4).copy()
    n = BITS[dst]
    if dst[0] == "u":
        return _le_bytes(((s + 2 ** 31) & 0xffffffff) >> (32 - n), n // 8)  # i32_to_u32 (wrapping add), then the top bits
    return _le_bytes(s >> (32 - n), n // 8)  # arithmetic shift


def expected(src, dst, planes, channels, nf):
    """planes[n_groups * channels, stride] -> uint8[n_groups, nf * channels * bytes]: frame by frame, channel by channel"""
    b = BYTES[dst]
    g = planes.shape[0] // channels
    conv = restate(src, dst, np.ascontiguousarray(planes[:, :nf]).ravel()).reshape(g, channels, nf, b)
    return conv.transpose(0, 2, 1, 3).reshape(g, nf * channels * b)


def sweep_inputs(src):
    if src == "f32":
        rng = np.random.default_rng(3)
        return np.concatenate([M.special_f32(), M.steps16(1), M.steps24(400, seed=5), (rng.standard_normal(1000) * 0.8).astype(np.float32)]).astype(np.float32)
    return M.inputs_i32()


# ---- running on either library -------------------------------------------------------------------------------------------------

class EmuDev:
    """the emulation's device memory is host memory"""

    def __init__(self, ctx):
        self.ctx = ctx

    def put(self, a):
        return np.ascontiguousarray(a).copy()

    def zeros(self, n, fill=0):
        return np.full(n, fill, np.uint8)

    def get(self, t):
        return t

    def addr(self, t):
        return t.ctypes.data


class GpuDev:
    def __init__(self, ctx):
        import torch
        self.ctx, self.torch = ctx, torch
        ctx.use_torch_stream()

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).ravel().copy()).cuda()

    def zeros(self, n, fill=0):
        return self.torch.full((n,), fill, dtype=self.torch.uint8, device="cuda")

    def get(self, t):
        self.torch.cuda.synchronize()
        return t.cpu().numpy()

    def addr(self, t):
        return t.data_ptr()


def _gpu_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on an MI355X (there is no CPU path)")
    return GpuDev(Context(0))


GUARD = 0xA5


def run_device(dev, src, dst, planes, channels, nf, group_pad=0, dst_offset=0, src_offset=0):
    """symaccel_pcm_convert_device on planes[n_groups * channels, stride] (src_offset: samples the first plane starts past a 64-byte
    boundary); returns uint8[n_groups, group bytes] and checks that nothing outside the groups' bytes was written"""
    g, stride = planes.shape[0] // channels, planes.shape[1]
    gb = nf * channels * BYTES[dst]
    pitch = gb + group_pad
    flat = np.concatenate([np.zeros(src_offset, planes.dtype), planes.ravel()])
    d_src = dev.put(flat)
    total = dst_offset + max(g, 1) * pitch + 64
    d_dst = dev.zeros(total, GUARD)
    pcm_convert_device(dev.ctx, dev.addr(d_src) + 4 * src_offset, FMT[src], stride, g, channels, nf, dev.addr(d_dst), FMT[dst], pitch, dst_offset=dst_offset)
    out = dev.get(d_dst)
    body = out[dst_offset:dst_offset + g * pitch].reshape(g, pitch) if g else np.zeros((0, pitch), np.uint8)
    assert np.all(out[:dst_offset] == GUARD) and np.all(out[dst_offset + g * pitch:] == GUARD), "bytes outside the output were written"
    assert np.all(body[:, gb:] == GUARD), "bytes between the groups were written"
    return body[:, :gb]


def planes_of(src, x, rows):
    """x cut into `rows` equal planes (the tail dropped)"""
    n = len(x) // rows
    return np.ascontiguousarray(x[:n * rows].reshape(rows, n))


# ---- constants -------------------------------------------------------------------------------------------------------------------

def check_sample_bytes(lib):
    assert [sample_bytes(f, lib) for f in (FMT_U8, FMT_S8, FMT_U16, FMT_S16, FMT_U24, FMT_S24, FMT_U32, FMT_S32, FMT_F32)] == [1, 1, 2, 2, 3, 3, 4, 4, 4]
    assert [FMT_U8, FMT_S8, FMT_U16, FMT_S16, FMT_U24, FMT_S24, FMT_U32, FMT_S32, FMT_F32] == list(range(1, 10))
    assert [sample_bytes(f, lib) for f in (0, 10, -1, 255, 1 << 20)] == [0, 0, 0, 0, 0]
    assert sample_bytes("s24", lib) == 3 and sample_bytes("F32", lib) == 4


def test_sample_bytes():
    check_sample_bytes(emu_library())


@pytest.mark.gpu
def test_gpu_sample_bytes():
    from symphonia_amd import default_library
    check_sample_bytes(default_library())


# ---- the two expectations agree ----------------------------------------------------------------------------------------------------

def fixture():
    z = np.load(GOLDEN)
    return z, z["in_f32"].view(np.float32), z["in_i32"]


@pytest.mark.parametrize("src,dst", PAIRS, ids=["%s_to_%s" % p for p in PAIRS])
def test_restatement_equals_the_reference_fixture(src, dst):
    z, xf, xi = fixture()
    want = z["%s_to_%s" % (src, dst)]
    got = restate(src, dst, xf if src == "f32" else xi)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%d of %d differ, first input %r: %r != %r" % (bad.size, len(want), (xf if src == "f32" else xi)[bad[0]], got[bad[0]], want[bad[0]])


def test_fixture_manifest_names_what_was_executed():
    z, xf, xi = fixture()
    man = json.loads(bytes(z["manifest"]).decode())
    assert sorted(e["pair"] for e in man["entries"]) == sorted("%s_to_%s" % p for p in PAIRS)
    for e in man["entries"]:
        assert e["ref"].startswith("symphonia-core/src/audio/conv.rs:") and e["cases"] == len(xf if e["pair"].startswith("f32") else xi)
    assert len(xf) > 4000 and len(xi) > 200


@pytest.mark.localref
def test_fixture_rederived_from_the_reference_tree():
    assert M.compare(M.generate(), dict(np.load(GOLDEN))) == []


# ---- the kernel --------------------------------------------------------------------------------------------------------------------

def check_fixture_through_kernel(dev, src, dst):
    z, xf, xi = fixture()
    x = xf if src == "f32" else xi
    got = run_device(dev, src, dst, x.reshape(1, -1), 1, len(x))
    assert np.array_equal(got.reshape(len(x), BYTES[dst]), z["%s_to_%s" % (src, dst)])


def check_sweep(dev, src, dst):
    """every sweep value, as mono (one plane), stereo and 5 channels (the planes are consecutive fifths of the sweep)"""
    x = sweep_inputs(src)
    for channels in (1, 2, 5):
        planes = planes_of(src, x, channels)
        nf = planes.shape[1]
        got = run_device(dev, src, dst, planes, channels, nf)
        want = expected(src, dst, planes, channels, nf)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s -> %s, %d channels: %d bytes differ, first at %d" % (src, dst, channels, bad.size, bad[0])


@pytest.mark.parametrize("src,dst", PAIRS, ids=["%s_to_%s" % p for p in PAIRS])
def test_fixture_through_the_kernel(emu_ctx, src, dst):
    check_fixture_through_kernel(EmuDev(emu_ctx), src, dst)


@pytest.mark.parametrize("src,dst", PAIRS, ids=["%s_to_%s" % p for p in PAIRS])
def test_every_step_and_boundary(emu_ctx, src, dst):
    check_sweep(EmuDev(emu_ctx), src, dst)


@pytest.mark.gpu
def test_gpu_fixture_and_every_step_and_boundary():
    dev = _gpu_dev()
    for src, dst in PAIRS:
        check_fixture_through_kernel(dev, src, dst)
        check_sweep(dev, src, dst)
    dev.ctx.close()


# the reference's own assertions (conv.rs `verify_*_from_sample`: MAX / MID / MIN of every source into every target), for the sources and
# targets this entry point has (f64 is neither)
LIMITS = {"u8": (255, 128, 0), "u16": (65535, 32768, 0), "u24": (16777215, 8388608, 0), "u32": (4294967295, 2147483648, 0),
          "s8": (127, 0, -128), "s16": (32767, 0, -32768), "s24": (8388607, 0, -8388608), "s32": (2147483647, 0, -2147483648)}


def check_reference_assertions(dev):
    for src, x in (("f32", np.array([1.0, 0.0, -1.0], np.float32)), ("s32", np.array([2 ** 31 - 1, 0, -2 ** 31], np.int64).astype(np.int32))):
        for dst in DESTS:
            got = run_device(dev, src, dst, x.reshape(1, 3), 1, 3).reshape(3, BYTES[dst])
            if dst == "f32":
                want = np.array([1.0 if src == "f32" else 2147483647.0 / 2147483648.0, 0.0, -1.0]).astype(np.float32)
                assert np.array_equal(got.view(np.float32).ravel(), want), (src, dst)
            else:
                assert np.array_equal(got, _le_bytes(np.array(LIMITS[dst], np.int64), BYTES[dst])), (src, dst)


def test_reference_max_mid_min_assertions(emu_ctx):
    check_reference_assertions(EmuDev(emu_ctx))


@pytest.mark.gpu
def test_gpu_reference_max_mid_min_assertions():
    dev = _gpu_dev()
    check_reference_assertions(dev)
    dev.ctx.close()


# ---- shapes ------------------------------------------------------------------------------------------------------------------------

FRAME_COUNTS = (0, 1, 2, 3, 4, 5, 15, 17, 63, 64, 65, 257, 1000, 1023, 1364, 2731, 4099)


def shape_case(src, rng, rows, stride):
    if src == "f32":
        return (rng.standard_normal((rows, stride)) * 0.6).astype(np.float32)
    return rng.integers(-2 ** 31, 2 ** 31, (rows, stride)).astype(np.int32)


def check_shapes(dev, lib, channels, quick=False):
    """channels x every destination: frame counts that are a multiple of no tile (down to 1 and 0), strides beyond the frame count
    (symaccel_row_stride among them), planes that start off a 16-byte boundary, gaps between the groups, an unaligned destination for the
    1- and 3-byte formats"""
    rng = np.random.default_rng(100 + channels)
    for di, dst in enumerate(DESTS):
        src = ("f32", "s32")[(di + channels) % 2]
        b = BYTES[dst]
        for ni, nf in enumerate(FRAME_COUNTS[::3] if quick else FRAME_COUNTS):
            groups = (1, 3, 2)[ni % 3]
            stride = (nf, nf + 5, int(lib.dll.symaccel_row_stride(nf)) + 4 * (ni % 2))[ni % 3]
            planes = shape_case(src, rng, groups * channels, stride)
            pad = ((0, 16, 7 * b)[ni % 3]) if b in (2, 4) else (0, 16, 7, 1)[ni % 4]
            off = b * (ni % 5) if b in (2, 4) else (0, 1, 2, 3, 5, 13)[(ni + di) % 6]
            got = run_device(dev, src, dst, planes, channels, nf, group_pad=pad, dst_offset=off, src_offset=(0, 1, 2, 3)[(ni + channels) % 4])
            assert np.array_equal(got, expected(src, dst, planes, channels, nf)), (src, dst, channels, nf, groups, stride, pad, off)


@pytest.mark.parametrize("channels", range(1, 9))
def test_shapes(emu_ctx, channels):
    check_shapes(EmuDev(emu_ctx), emu_ctx.lib, channels)


@pytest.mark.gpu
@pytest.mark.parametrize("channels", range(1, 9))
def test_gpu_shapes(channels):
    dev = _gpu_dev()
    check_shapes(dev, dev.ctx.lib, channels)
    dev.ctx.close()


def check_many_groups(dev):
    rng = np.random.default_rng(9)
    for src, dst, channels, nf, groups in (("f32", "s16", 2, 1024, 700), ("s32", "s24", 2, 4096 + 12, 37), ("f32", "u8", 6, 300, 513), ("s32", "s16", 1, 7, 3000),
                                           ("f32", "s24", 8, 1152, 129), ("f32", "f32", 2, 2048, 64)):
        planes = shape_case(src, rng, groups * channels, nf + (8 if groups % 2 else 0))
        got = run_device(dev, src, dst, planes, channels, nf)
        assert np.array_equal(got, expected(src, dst, planes, channels, nf)), (src, dst, channels, nf, groups)


def test_many_groups(emu_ctx):
    check_many_groups(EmuDev(emu_ctx))


@pytest.mark.gpu
def test_gpu_many_groups():
    dev = _gpu_dev()
    check_many_groups(dev)
    dev.ctx.close()


def check_in_place_planar(dev):
    """the one overlap that is allowed: a planar conversion between 4-byte formats over itself"""
    rng = np.random.default_rng(11)
    for src, dst in (("f32", "s32"), ("s32", "f32"), ("f32", "u32"), ("s32", "s32")):
        planes = shape_case(src, rng, 5, 1003)
        d = dev.put(planes)
        pcm_convert_device(dev.ctx, dev.addr(d), FMT[src], 1003, 5, 1, 1001, dev.addr(d), FMT[dst], 1003 * 4)
        got = dev.get(d).view(np.uint8).reshape(5, 1003 * 4)
        assert np.array_equal(got[:, :1001 * 4], expected(src, dst, planes, 1, 1001)), (src, dst)
        assert np.array_equal(got[:, 1001 * 4:], planes.view(np.uint8).reshape(5, -1)[:, 1001 * 4:])


def test_in_place_planar(emu_ctx):
    check_in_place_planar(EmuDev(emu_ctx))


@pytest.mark.gpu
def test_gpu_in_place_planar():
    dev = _gpu_dev()
    check_in_place_planar(dev)
    dev.ctx.close()


# ---- the host form -----------------------------------------------------------------------------------------------------------------

def check_host_form(ctx):
    rng = np.random.default_rng(13)
    for src, dst, channels, nf, groups, stride in (("f32", "s16", 2, 1024, 9, 1024), ("s32", "s24", 3, 777, 4, 800), ("f32", "u8", 1, 5, 2, 5),
                                                   ("s32", "f32", 8, 4608, 2, 4608), ("f32", "s32", 2, 0, 3, 4), ("f32", "u24", 5, 1, 1, 1)):
        planes = shape_case(src, rng, groups * channels, stride)
        got = pcm_convert(ctx, planes, dst, channels=channels, n_frames=nf)
        assert got.shape == (groups, nf * channels * BYTES[dst])
        assert np.array_equal(got, expected(src, dst, planes, channels, nf)), (src, dst, channels, nf)


def test_host_form(emu_ctx):
    check_host_form(emu_ctx)


def test_host_form_in_chunks(emu_ctx):
    """more input than one staging chunk holds (32 MiB): the frame axis is cut, every group's output is written in pieces"""
    rng = np.random.default_rng(14)
    planes = (rng.standard_normal((6, 1_500_001)) * 0.5).astype(np.float32)
    got = pcm_convert(emu_ctx, planes, "s24", channels=3)
    assert np.array_equal(got, expected("f32", "s24", planes, 3, planes.shape[1]))


@pytest.mark.gpu
def test_gpu_host_form():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on an MI355X (there is no CPU path)")
    with Context(0) as ctx:
        check_host_form(ctx)
        rng = np.random.default_rng(14)
        planes = (rng.standard_normal((6, 1_500_001)) * 0.5).astype(np.float32)
        assert np.array_equal(pcm_convert(ctx, planes, "s24", channels=3), expected("f32", "s24", planes, 3, planes.shape[1]))


# ---- what is refused ---------------------------------------------------------------------------------------------------------------

def check_refusals(dev):
    ctx = dev.ctx
    src = dev.put(np.zeros((8, 64), np.float32))
    dst = dev.zeros(8 * 64 * 4 + 64)
    s, d = dev.addr(src), dev.addr(dst)

    def refused(*args):
        with pytest.raises(SymaccelError) as e:
            pcm_convert_device(ctx, *args)
        assert e.value.status == -1, args

    pcm_convert_device(ctx, s, FMT_F32, 64, 4, 2, 64, d, FMT_S16, 256)  # the baseline is fine
    refused(s, 0, 64, 4, 2, 64, d, FMT_S16, 256)            # unknown source format
    refused(s, FMT_S16, 64, 4, 2, 64, d, FMT_S16, 256)      # a source the library never produces
    refused(s, FMT_F32, 64, 4, 2, 64, d, 10, 256)           # unknown destination format
    refused(s, FMT_F32, 64, 4, 2, 64, d, 0, 256)
    refused(s, FMT_F32, 64, 8, 0, 64, d, FMT_S16, 256)      # channels outside 1..8
    refused(s, FMT_F32, 64, 0, 9, 64, d, FMT_S16, 2000)
    refused(s, FMT_F32, 63, 4, 2, 64, d, FMT_S16, 256)      # planes that overlap their neighbours
    refused(s, FMT_F32, 64, 4, 2, 64, d, FMT_S16, 255)      # dst_group_bytes smaller than one group
    refused(s, FMT_F32, 64, 4, 2, 64, d + 1, FMT_S16, 256)  # a 2-byte format off its alignment
    refused(s, FMT_F32, 64, 4, 2, 64, d + 2, FMT_S32, 512)
    refused(s, FMT_F32, 64, 4, 2, 60, d, FMT_S16, 241)      # groups that would fall off it
    refused(s + 2, FMT_F32, 64, 4, 2, 60, d, FMT_S16, 256)  # source samples off their alignment
    refused(s, FMT_F32, 64, 4, 2, 64, s + 64, FMT_S16, 256)  # overlapping
    refused(s, FMT_F32, 64, 4, 2, 64, s, FMT_S16, 256)
    refused(s, FMT_F32, 64, 4, 2, 64, s, FMT_F32, 512)      # in place, but interleaving
    refused(s, FMT_F32, 64, 8, 1, 64, s, FMT_S16, 128)      # in place, but narrower
    refused(s, FMT_F32, 64, 8, 1, 60, s, FMT_S32, 240)      # in place, but another pitch
    refused(None, FMT_F32, 64, 4, 2, 64, d, FMT_S16, 256)
    refused(s, FMT_F32, 64, 4, 2, 64, None, FMT_S16, 256)
    pcm_convert_device(ctx, s, FMT_F32, 64, 0, 2, 64, d, FMT_S16, 256)  # nothing to do is not an error
    pcm_convert_device(ctx, s, FMT_F32, 64, 4, 2, 0, d, FMT_S24, 0)
    pcm_convert_device(ctx, s, FMT_F32, 64, 4, 2, 64, d + 3, FMT_S24, 385)  # the 3-byte formats go anywhere
    dev.get(dst)


def test_refusals(emu_ctx):
    check_refusals(EmuDev(emu_ctx))
    with pytest.raises(SymaccelError):
        pcm_convert(emu_ctx, np.zeros((2, 8), np.float32), 10, channels=2)
    with pytest.raises(ValueError):
        pcm_convert(emu_ctx, np.zeros((3, 8), np.float32), "s16", channels=2)
    with pytest.raises(ValueError):
        pcm_convert(emu_ctx, np.zeros((2, 8), np.float64), "s16", channels=2)


@pytest.mark.gpu
def test_gpu_refusals():
    dev = _gpu_dev()
    check_refusals(dev)
    dev.ctx.close()
