"""TEST ONLY.  The Layer I and Layer II dequantisations (symphonia-bundle-mp3/src/layer1/mod.rs:51-60, 156-159; layer2/mod.rs:198-213,
341-346) in numpy float32, one numpy operation per operation of the reference, on the inputs symaccel_mpa12_decode takes.  The
tables are the reference's own bit patterns (tests/golden/mpa12/tables.npz, read out of the interpreted reference by
tools/make_mpa12_fixtures.py); expected PCM is oracle.mp3_polyphase of what this file returns.  tests/test_mpa12.py pins the file to
the reference: for the fixtures' codes and records its PCM must be what Layer1::decode / Layer2::decode produced."""
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "mpa12"
LAYER1, LAYER2 = 1, 2
N_FRAMES = {LAYER1: 12, LAYER2: 36}
RECORD_BYTES = {LAYER1: 64, LAYER2: 128}
F32 = np.float32

_tables = None


def tables():
    """{"factor": f32[16], "scalefactors": f32[64], "c": f32[17], "d": f32[17], "width": int[17]} from the fixture"""
    global _tables
    if _tables is None:
        t = np.load(GOLDEN / "tables.npz")
        bits, grouping, nlevels = t["class_bits_grouping_nlevels"].astype(np.int64).T
        # layer2/mod.rs:183: nlevels.next_power_of_two().trailing_zeros()
        width = np.where(grouping != 0, [int(n - 1).bit_length() for n in nlevels], bits)
        _tables = {"factor": t["factor"].view(F32), "scalefactors": t["scalefactors"].view(F32), "c": t["class_cd"][:, 0].copy().view(F32),
                   "d": t["class_cd"][:, 1].copy().view(F32), "width": width}
    return _tables


def packed_tables():
    """the layout of SYMACCEL_TABLE_MPA12: FACTOR[16] | SCALEFACTORS[64] | 17 x {c, d, (float) sample width}"""
    t = tables()
    cls = np.stack([t["c"], t["d"], t["width"].astype(F32)], 1).ravel()
    return np.concatenate([t["factor"], t["scalefactors"], cls]).astype(F32)


def sign_extend(value, width):
    """util/bits.rs sign_extend_leq32_to_i32 on int64 arrays"""
    value = value & ((1 << width) - 1)
    return np.where(value >> (width - 1) != 0, value - (1 << width), value)


def record_ok(layer, rec):
    """False for a record symaccel_mpa12_decode marks with status 1"""
    rec = np.asarray(rec, np.uint8)
    if layer == LAYER1:
        return not ((rec[:32] == 1).any() or (rec[:32] > 15).any() or (rec[32:] > 63).any())
    return not ((rec[:32] > 17).any() or (rec[32:] > 63).any())


def dequantize(layer, codes, rec):
    """codes[32][n_frames] u16 and the record of ONE channel-packet -> samples[32 * n_frames] f32 (samples[ch] of the reference)"""
    t, nf = tables(), N_FRAMES[layer]
    codes = np.asarray(codes).reshape(32, nf).astype(np.int64)
    rec = np.asarray(rec, np.uint8)
    out = np.zeros((32, nf), F32)  # let mut samples = [[0f32; ..]; 2]
    if not record_ok(layer, rec):
        return out.ravel()
    for sb in range(32):
        alloc = int(rec[sb])
        if alloc == 0:
            continue
        if layer == LAYER1:
            bits = alloc
            raw = codes[sb] & ((1 << bits) - 1)
            a = sign_extend(raw ^ (1 << (bits - 1)), bits)                     # layer1/mod.rs:53-56
            sample = t["factor"][bits] * (a + 1).astype(F32)                   # :59
            out[sb] = t["scalefactors"][rec[32 + sb]] * sample                 # :159
        else:
            k = alloc - 1
            bits = int(t["width"][k])
            raw = codes[sb] & ((1 << bits) - 1)
            divisor = F32(1 << (bits - 1))                                     # layer2/mod.rs:198
            a = sign_extend(raw ^ (1 << (bits - 1)), bits)                     # :204-207
            s = a.astype(F32) / divisor                                        # :210
            s = s + t["d"][k]                                                  # :213 (the sum ...
            tr = t["c"][k] * s                                                 #       ... then the product)
            scalefac = t["scalefactors"][rec[32 + sb + 32 * (np.arange(36) // 12)]]  # :341: scalefacs[ch][gr / 4][sb], gr = j / 3
            out[sb] = scalefac * tr                                            # :344-346
    assert out.dtype == F32
    return out.ravel()


def dequantize_batch(layer, codes, rec):
    """codes[chains][packets][32][n_frames], rec[chains][packets][record bytes] -> f32[chains][packets][32 * n_frames]"""
    nch, npk = codes.shape[:2]
    out = np.zeros((nch, npk, 32 * N_FRAMES[layer]), F32)
    for c in range(nch):
        for p in range(npk):
            out[c, p] = dequantize(layer, codes[c, p], rec[c, p])
    return out


def synthesize(layer, x, vvec, vfront):
    """oracle.mp3_polyphase over x[chains][packets][32 * n_frames] with the state carried: (pcm, vvec, vfront)"""
    import oracle
    nch, npk = x.shape[:2]
    pcm = np.zeros_like(x)
    vvec, vfront = np.array(vvec, F32, copy=True), np.array(vfront, np.int32, copy=True)
    for c in range(nch):
        v, f = vvec[c], int(vfront[c])
        for p in range(npk):
            pcm[c, p], v, f = oracle.mp3_polyphase(v, f, N_FRAMES[layer], x[c, p])
        vvec[c], vfront[c] = v, f
    return pcm, vvec, vfront


def decode(layer, codes, rec, vvec, vfront):
    """what symaccel_mpa12_decode must return: (pcm, vvec, vfront, status)"""
    x = dequantize_batch(layer, codes, rec)
    status = np.array([[0 if record_ok(layer, rec[c, p]) else 1 for p in range(codes.shape[1])] for c in range(codes.shape[0])], np.uint8).reshape(codes.shape[:2])
    return synthesize(layer, x, vvec, vfront) + (status,)
