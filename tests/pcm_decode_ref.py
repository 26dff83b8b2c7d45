"""A numpy restatement of symphonia-codec-pcm's PcmDecoder (lib.rs:50-118, 154-181, 318-411) and of the 10 x 9 FromSample conversions its
buffers can be delivered through (symphonia-core/src/audio/conv.rs:461-621), written from the reference's text, one formula per line of
conv.rs -- not through the left-justified i32 the kernel carries, so that the kernel's shortcut is checked and not repeated.

tests/test_pcm_decode.py pins it to tests/golden/pcm_decode.npz (the reference's own decoder under the interpreter) and, exhaustively,
to scalar forms of the reference's arithmetic."""
import numpy as np

# name -> (coded bytes, kind, big-endian, native family); kind: "s" / "u" integer, "f" float, "alaw", "mulaw"
CODECS = {
    "s32le": (4, "s", False, "s32"), "s32be": (4, "s", True, "s32"), "s24le": (3, "s", False, "s24"), "s24be": (3, "s", True, "s24"),
    "s16le": (2, "s", False, "s16"), "s16be": (2, "s", True, "s16"), "s8": (1, "s", False, "s8"),
    "u32le": (4, "u", False, "u32"), "u32be": (4, "u", True, "u32"), "u24le": (3, "u", False, "u24"), "u24be": (3, "u", True, "u24"),
    "u16le": (2, "u", False, "u16"), "u16be": (2, "u", True, "u16"), "u8": (1, "u", False, "u8"),
    "f32le": (4, "f", False, "f32"), "f32be": (4, "f", True, "f32"), "f64le": (8, "f", False, "f64"), "f64be": (8, "f", True, "f64"),
    "alaw": (1, "alaw", False, "s16"), "mulaw": (1, "mulaw", False, "s16"),
}
NAMES = tuple(CODECS)  # in the order of SYMACCEL_PCM_* (1..20)
FAMILIES = ("s8", "s16", "s24", "s32", "u8", "u16", "u24", "u32", "f32", "f64")
NATIVE_DTYPE = {"s8": np.int8, "s16": np.int16, "s24": np.int32, "s32": np.int32, "u8": np.uint8, "u16": np.uint16, "u24": np.uint32, "u32": np.uint32,
                "f32": np.float32, "f64": np.float64}
WIDTH = {"s8": 8, "s16": 16, "s24": 24, "s32": 32, "u8": 8, "u16": 16, "u24": 24, "u32": 32, "f32": 32, "f64": 64}
DESTS = ("u8", "s8", "u16", "s16", "u24", "s24", "u32", "s32", "f32")
DEST_BYTES = {"u8": 1, "s8": 1, "u16": 2, "s16": 2, "u24": 3, "s24": 3, "u32": 4, "s32": 4, "f32": 4}
MAX_CHANNELS, TILE_BYTES = 8, 16384


def coded_bytes(codec):
    return CODECS[codec][0]


def native_bytes(codec):
    return np.dtype(NATIVE_DTYPE[CODECS[codec][3]]).itemsize


def legal_shifts(codec):
    """the shifts PcmDecoder::try_new can arrive at and `<<` takes (lib.rs:264-307): 0 .. width - 1 for the integer codecs, 0 otherwise"""
    _, kind, _, fam = CODECS[codec]
    return range(WIDTH[fam]) if kind in "su" else range(1)


def tile_frames(channels, coded, out):
    """pcm_decode_tile_frames of csrc/symaccel_internal.h: the frames of a kernel tile"""
    return ((TILE_BYTES - 256) // (channels * max(coded, out))) & ~15


def _sext(v, bits):
    v = np.asarray(v, np.int64) & ((1 << bits) - 1)
    return np.where(v >> (bits - 1), v - (1 << bits), v)


def alaw_to_linear(a):
    """lib.rs:154-167 on an array of codes"""
    a = np.asarray(a, np.int64) ^ 0x55
    t = (a & 0x0f) << 4
    seg = (a & 0x70) >> 4
    t = np.where(seg == 0, t + 0x8, np.where(seg == 1, t + 0x108, (t + 0x108) << np.maximum(seg - 1, 0)))
    return np.where(a & 0x80, t, -t)


def mulaw_to_linear(mu):
    """lib.rs:169-181"""
    mu = ~np.asarray(mu, np.int64) & 0xff
    t = (((mu & 0x0f) << 3) + 0x84) << ((mu & 0x70) >> 4)
    return np.where(mu & 0x80, 0x84 - t, t - 0x84)


def decode_samples(coded, codec, shift=0):
    """coded: uint8[n, coded bytes] -> the n native samples (NATIVE_DTYPE of the codec's family)"""
    cb, kind, be, fam = CODECS[codec]
    coded = np.asarray(coded, np.uint8).reshape(-1, cb)
    le = coded[:, ::-1] if be else coded
    if kind == "f":
        return np.ascontiguousarray(le).view("<f4" if cb == 4 else "<f8").ravel().copy()
    v = np.zeros(len(le), np.int64)
    for k in range(cb):
        v |= le[:, k].astype(np.int64) << (8 * k)
    if kind == "alaw":
        return alaw_to_linear(v).astype(np.int16)
    if kind == "mulaw":
        return mulaw_to_linear(v).astype(np.int16)
    w = 8 * cb
    if w == 24:
        # lib.rs:336-360: read_[be_]x24() << 8 in 32 bits, << shift there, then x24::from(x >> 8) (conv.rs:528, 583), which clamps to 24 bits
        x = ((v << 8) << shift) & 0xffffffff
        if kind == "s":
            return np.clip(_sext(x, 32) >> 8, -(1 << 23), (1 << 23) - 1).astype(np.int32)
        return np.minimum(x >> 8, 0xffffff).astype(np.uint32)
    x = (v << shift) & ((1 << w) - 1)  # `<<` drops the high bits in the width of the type
    return (_sext(x, w) if kind == "s" else x).astype(NATIVE_DTYPE[fam])


def decode(packets, codec, channels, frames, shift=0):
    """packets: uint8[n, >= frames * channels * coded bytes] -> the native planes [n, channels, frames]"""
    cb = coded_bytes(codec)
    packets = np.asarray(packets, np.uint8)
    n = packets.shape[0]
    s = decode_samples(np.ascontiguousarray(packets[:, :frames * channels * cb]).reshape(-1, cb), codec, shift)
    return np.ascontiguousarray(s.reshape(n, frames, channels).transpose(0, 2, 1))


def frames_of(length, codec, channels):
    """lib.rs:320: complete frames of a packet of `length` bytes"""
    return length // (coded_bytes(codec) * channels)


# ---- conv.rs:461-621 ---------------------------------------------------------------------------------------------------------------------

def _le(v, nbytes):
    return (np.asarray(v, np.int64) & 0xffffffff).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :nbytes].copy()


def _f32_bytes(v):
    return np.asarray(v, np.float32).view(np.uint8).reshape(-1, 4).copy()


def _as_int(v, lo, hi):
    """Rust's `v as <integer>`: toward zero, saturating, NaN -> 0"""
    v = np.asarray(v, np.float64)
    out = np.zeros(v.shape, np.int64)
    ok = ~np.isnan(v)
    out[ok] = np.trunc(np.clip(v[ok], float(lo), float(hi))).astype(np.int64)
    return out


def f64_as_f32_bits(x):
    """`s as f32` (conv.rs:621): nearest-even; a NaN keeps its sign and the top 22 bits of its payload and becomes quiet"""
    x = np.asarray(x, np.float64)
    bits = x.view(np.uint64)
    with np.errstate(over="ignore", invalid="ignore"):
        out = x.astype(np.float32).view(np.uint32).copy()
    nan = np.isnan(x)
    out[nan] = ((bits[nan] >> np.uint64(32)) & np.uint64(0x80000000)).astype(np.uint32) | np.uint32(0x7fc00000) | ((bits[nan] >> np.uint64(29)) & np.uint64(0x3fffff)).astype(np.uint32)
    return out


def convert(fam, dst, x):
    """FromSample<fam> for dst on an array of native samples -> uint8[n, bytes of dst] (24-bit: three little-endian bytes)"""
    nb, n = DEST_BYTES[dst], (int(dst[1:]) if dst != "f32" else 0)
    if fam in ("f32", "f64"):
        ft = np.float32 if fam == "f32" else np.float64
        x = np.asarray(x, ft)
        if dst == "f32":
            return x.view(np.uint8).reshape(-1, 4).copy() if fam == "f32" else f64_as_f32_bits(x).view(np.uint8).reshape(-1, 4).copy()  # conv.rs:606, 621
        with np.errstate(invalid="ignore", over="ignore"):
            c = np.where(x > ft(1.0), ft(1.0), x)  # util.rs:258-275: two comparisons, a NaN fails both
            c = np.where(c < ft(-1.0), ft(-1.0), c).astype(ft)
            if dst[0] == "u":  # conv.rs:596-599, 611-614
                one = (c + ft(1.0)).astype(ft)
                v = one.astype(np.float64) * 2147483648.0 if n == 32 else (one * ft(2.0 ** (n - 1))).astype(ft)
                if n == 24:
                    return _le(np.minimum(_as_int(v, 0, 2 ** 32 - 1), 0xffffff), 3)  # `as u32`, then u24::from clamps
                return _le(_as_int(v, 0, 2 ** n - 1), nb)
            v = c.astype(np.float64) * 2147483648.0 if n == 32 else (c * ft(2.0 ** (n - 1))).astype(ft)  # conv.rs:601-604, 616-619
            if n == 24:
                return _le(np.clip(_as_int(v, -2 ** 31, 2 ** 31 - 1), -2 ** 23, 2 ** 23 - 1), 3)  # `as i32`, then i24::from clamps
            return _le(_as_int(v, -2 ** (n - 1), 2 ** (n - 1) - 1), nb)
    w = WIDTH[fam]
    s = np.asarray(x).astype(np.int64)
    if fam[0] == "s":
        if dst == "f32":
            if w == 32:
                return _f32_bytes((s.astype(np.float64) / 2147483648.0).astype(np.float32))  # conv.rs:531
            return _f32_bytes(s.astype(np.float32) / np.float32(2.0 ** (w - 1)))  # conv.rs:471, 491, 511
        if dst[0] == "u":
            if w == 24:
                u = ((s << 8) + 0x80000000) & 0xffffffff  # i24_to_u32, conv.rs:497-499
                return _le(u >> (32 - n), nb)  # conv.rs:501-504
            u = (s + (1 << (w - 1))) & ((1 << w) - 1)  # i8_to_u8, i16_to_u16, i32_to_u32
            return _le(u << (n - w) if n >= w else u >> (w - n), nb)  # conv.rs:461-464, 481-484, 521-524
        return _le(s << (n - w) if n >= w else s >> (w - n), nb)  # conv.rs:466-469, 486-489, 506-509, 526-529
    if dst == "f32":
        if w == 32:
            return _f32_bytes(((s.astype(np.float64) / 2147483648.0) - 1.0).astype(np.float32))  # conv.rs:591
        return _f32_bytes(((s.astype(np.float32) / np.float32(2.0 ** (w - 1))).astype(np.float32) - np.float32(1.0)).astype(np.float32))  # conv.rs:546, 561, 576
    if dst[0] == "u":
        return _le(s << (n - w) if n >= w else s >> (w - n), nb)  # conv.rs:536-539, 551-554, 566-569, 581-584
    i = _sext(s - (1 << (w - 1)), w)  # wrapping_sub(0x80..) as the signed type
    return _le(i << (n - w) if n >= w else i >> (w - n), nb)  # conv.rs:541-544, 556-559, 571-574, 586-589


def interleave(planes, fam, dst):
    """native planes [n, channels, frames] -> uint8[n, frames * channels * bytes of dst]: frame by frame, channel by channel"""
    n, ch, nf = planes.shape
    b = DEST_BYTES[dst]
    return convert(fam, dst, np.ascontiguousarray(planes).ravel()).reshape(n, ch, nf, b).transpose(0, 2, 1, 3).reshape(n, nf * ch * b)


# ---- scalar forms, for the exhaustive pins -------------------------------------------------------------------------------------------------

def alaw_scalar(a):
    a ^= 0x55
    t = (a & 0x0f) << 4
    seg = (a & 0x70) >> 4
    t = t + 8 if seg == 0 else t + 0x108 if seg == 1 else (t + 0x108) << (seg - 1)
    assert -32768 <= t <= 32767
    return t if a & 0x80 else -t


def mulaw_scalar(mu):
    mu = ~mu & 0xff
    t = ((mu & 0x0f) << 3) + 0x84
    t <<= (mu & 0x70) >> 4
    assert -32768 <= t <= 32767
    return 0x84 - t if mu & 0x80 else t - 0x84


def int_scalar(value, width, signed, shift):
    """(read << shift) in a `width`-bit type: `value` is the read sample"""
    x = (value << shift) & ((1 << width) - 1)
    return x - (1 << width) if signed and x >> (width - 1) else x
