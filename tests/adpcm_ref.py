"""A numpy restatement of symphonia-codec-adpcm's block decoders (codec_ms.rs, codec_ima_wav.rs, codec_ima_qt.rs, common_ima.rs), written
from the contract and not from the kernel: vectorised ACROSS blocks (a step of the loop is one nibble of every block), serial inside a
block, and with the i32 wrapping of the reference's release build written out -- every product and sum that can leave 32 bits is taken
modulo 2^32 in int64 and folded back to a signed value, every division by 256 truncates toward zero."""
import numpy as np

MS, IMA_WAV, IMA_QT = 1, 2, 3
CODECS = {"ms": MS, "ima_wav": IMA_WAV, "ima_qt": IMA_QT}

IMA_INDEX = np.array([-1, -1, -1, -1, 2, 4, 6, 8, -1, -1, -1, -1, 2, 4, 6, 8], np.int64)
IMA_STEP = np.array([7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
                     157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411,
                     1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493,
                     10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767], np.int64)
MS_ADAPT = np.array([230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230], np.int64)
MS_C1 = np.array([256, 512, 0, 192, 240, 460, 392], np.int64)
MS_C2 = np.array([0, -256, 0, 64, 0, -208, -232], np.int64)


def block_bytes(codec, channels, fpb):
    """bytes of a block; 0 for the shapes the device decoder refuses (the table of the header)"""
    if channels not in (1, 2) or fpb <= 0 or fpb > 1 << 20:
        return 0
    if codec == MS:
        if fpb < 2 or (channels == 1 and fpb % 2):
            return 0
        return 6 + fpb // 2 if channels == 1 else 12 + fpb
    if codec == IMA_WAV:
        if channels == 1:
            return 0 if fpb % 2 == 0 else 4 + (fpb - 1) // 2
        return 0 if (fpb - 1) % 8 else 7 + fpb
    if codec == IMA_QT:
        return 34 * channels if fpb == 64 else 0
    return 0


def wrap32(v):
    """an int64 value as the i32 a wrapping operation leaves"""
    return ((np.asarray(v, np.int64) + (1 << 31)) & 0xffffffff) - (1 << 31)


def div256(v):
    """Rust's v / 256 on i32: toward zero"""
    v = np.asarray(v, np.int64)
    return np.where(v < 0, -((-v) >> 8), v >> 8)


def i16(lo, hi):
    v = lo.astype(np.int64) | (hi.astype(np.int64) << 8)
    return np.where(v >= 32768, v - 65536, v)


class MsState:
    def __init__(self, pi, delta, s1, s2):
        self.bad = pi > 6
        pi = np.where(self.bad, 0, pi)
        self.c1, self.c2, self.delta, self.s1, self.s2 = MS_C1[pi], MS_C2[pi], delta, s1, s2

    def nibble(self, n):
        n = n.astype(np.int64)
        sn = np.where(n & 8, n - 16, n)
        pred = wrap32(div256(self.s1 * self.c1 + self.s2 * self.c2) + wrap32(sn * self.delta))
        self.s2 = self.s1
        self.s1 = np.clip(pred, -32768, 32767)
        self.delta = np.maximum(16, div256(wrap32(MS_ADAPT[n] * self.delta)))
        return self.s1


class ImaState:
    def __init__(self, pred, idx, bad):
        self.pred, self.idx, self.bad = pred, idx, bad

    def nibble(self, n):
        n = n.astype(np.int64)
        diff = ((2 * (n & 7) + 1) * IMA_STEP[self.idx]) >> 3
        self.pred = np.clip(np.where(n & 8, self.pred - diff, self.pred + diff), -32768, 32767)
        self.idx = np.clip(self.idx + IMA_INDEX[n], 0, 88)
        return self.pred


def decode(blocks, codec, channels, fpb):
    """blocks uint8[n, >= block bytes] -> (pcm int32[n, channels, fpb] left-justified, status uint8[n]); a block with a non-zero status
    is all zeros"""
    codec = CODECS[codec] if isinstance(codec, str) else codec
    nbytes = block_bytes(codec, channels, fpb)
    if nbytes == 0:
        raise ValueError("refused shape")
    b = np.asarray(blocks, np.uint8)
    assert b.ndim == 2 and b.shape[1] >= nbytes
    n = b.shape[0]
    out = np.zeros((n, channels, fpb), np.int64)
    status = np.zeros(n, np.uint8)
    lo, hi = (lambda x: x & 15), (lambda x: x >> 4)
    if codec == MS:
        if channels == 1:
            st = [MsState(b[:, 0].astype(np.int64), i16(b[:, 1], b[:, 2]), i16(b[:, 3], b[:, 4]), i16(b[:, 5], b[:, 6]))]
        else:
            st = [MsState(b[:, c].astype(np.int64), i16(b[:, 2 + 2 * c], b[:, 3 + 2 * c]), i16(b[:, 6 + 2 * c], b[:, 7 + 2 * c]),
                          i16(b[:, 10 + 2 * c], b[:, 11 + 2 * c])) for c in range(2)]
        for c in range(channels):
            out[:, c, 0], out[:, c, 1] = st[c].s2, st[c].s1
            status[st[c].bad] = 1
        if channels == 1:
            for k in range(1, fpb // 2):
                byte = b[:, 6 + k]
                out[:, 0, 2 * k] = st[0].nibble(hi(byte))
                out[:, 0, 2 * k + 1] = st[0].nibble(lo(byte))
        else:
            for f in range(2, fpb):
                byte = b[:, 12 + f]
                out[:, 0, f] = st[0].nibble(hi(byte))
                out[:, 1, f] = st[1].nibble(lo(byte))
    elif codec == IMA_WAV:
        st = []
        for c in range(channels):
            idx = b[:, 4 * c + 2].astype(np.int64)
            st.append(ImaState(i16(b[:, 4 * c], b[:, 4 * c + 1]), np.minimum(idx, 88), idx > 88))
            out[:, c, 0] = st[c].pred
            status[st[c].bad] = 2
        if channels == 1:
            for k in range((fpb - 1) // 2):
                byte = b[:, 4 + k]
                out[:, 0, 1 + 2 * k] = st[0].nibble(lo(byte))
                out[:, 0, 2 + 2 * k] = st[0].nibble(hi(byte))
        else:
            for k in range(fpb - 1):
                c, off, j = (k // 4) & 1, (k // 8) * 8, k % 4
                byte = b[:, 8 + k]
                out[:, c, 1 + off + 2 * j] = st[c].nibble(lo(byte))
                out[:, c, 2 + off + 2 * j] = st[c].nibble(hi(byte))
    else:
        for c in range(channels):
            h = (b[:, 34 * c].astype(np.int64) << 8) | b[:, 34 * c + 1]
            p = h & 0xff80
            s = ImaState(np.where(p >= 32768, p - 65536, p), np.minimum(h & 0x7f, 88), np.zeros(n, bool))
            for k in range(32):
                byte = b[:, 34 * c + 2 + k]
                out[:, c, 2 * k] = s.nibble(lo(byte))
                out[:, c, 2 * k + 1] = s.nibble(hi(byte))
    out[status != 0] = 0
    return wrap32(out << 16).astype(np.int32), status


def decode_scalar(block, codec, channels, fpb):
    """One block, plain Python integers, statement by statement after the reference: the cross-check of the vectorised form."""
    codec = CODECS[codec] if isinstance(codec, str) else codec
    w = lambda v: ((v + (1 << 31)) & 0xffffffff) - (1 << 31)
    tdiv = lambda v: -((-v) // 256) if v < 0 else v // 256
    s16 = lambda lo_, hi_: ((lo_ | hi_ << 8) ^ 0x8000) - 0x8000
    clamp = lambda v: max(-32768, min(32767, v))
    bts = [int(x) for x in block]
    out = [[0] * fpb for _ in range(channels)]

    def ms_nib(s, nib):
        sn = nib - 16 if nib & 8 else nib
        pred = w(tdiv(s["s1"] * s["c1"] + s["s2"] * s["c2"]) + w(sn * s["d"]))
        s["s2"], s["s1"] = s["s1"], clamp(pred)
        s["d"] = max(16, tdiv(w(int(MS_ADAPT[nib]) * s["d"])))
        return s["s1"]

    def ima_nib(s, nib):
        diff = ((2 * (nib & 7) + 1) * int(IMA_STEP[s["i"]])) >> 3
        s["p"] = clamp(s["p"] - diff if nib & 8 else s["p"] + diff)
        s["i"] = max(0, min(88, s["i"] + int(IMA_INDEX[nib])))
        return s["p"]

    if codec == MS:
        st = []
        for c in range(channels):
            pi = bts[c]
            if pi > 6:
                return None, 1
            o = channels + 2 * c
            st.append({"c1": int(MS_C1[pi]), "c2": int(MS_C2[pi]), "d": s16(bts[o], bts[o + 1]), "s1": s16(bts[o + 2 * channels], bts[o + 2 * channels + 1]),
                       "s2": s16(bts[o + 4 * channels], bts[o + 4 * channels + 1])})
            out[c][0], out[c][1] = st[c]["s2"], st[c]["s1"]
        pos = 7 * channels
        if channels == 1:
            for k in range(1, fpb // 2):
                out[0][2 * k] = ms_nib(st[0], bts[pos] >> 4)
                out[0][2 * k + 1] = ms_nib(st[0], bts[pos] & 15)
                pos += 1
        else:
            for f in range(2, fpb):
                out[0][f] = ms_nib(st[0], bts[pos] >> 4)
                out[1][f] = ms_nib(st[1], bts[pos] & 15)
                pos += 1
    elif codec == IMA_WAV:
        st = []
        for c in range(channels):
            if bts[4 * c + 2] > 88:
                return None, 2
            st.append({"p": s16(bts[4 * c], bts[4 * c + 1]), "i": bts[4 * c + 2]})
            out[c][0] = st[c]["p"]
        pos = 4 * channels
        if channels == 1:
            for k in range((fpb - 1) // 2):
                out[0][1 + 2 * k] = ima_nib(st[0], bts[pos] & 15)
                out[0][2 + 2 * k] = ima_nib(st[0], bts[pos] >> 4)
                pos += 1
        else:
            for k in range(fpb - 1):
                c, off, j = (k // 4) & 1, (k // 8) * 8, k % 4
                out[c][1 + off + 2 * j] = ima_nib(st[c], bts[pos] & 15)
                out[c][2 + off + 2 * j] = ima_nib(st[c], bts[pos] >> 4)
                pos += 1
    else:
        pos = 0
        for c in range(channels):
            h = bts[pos] << 8 | bts[pos + 1]
            s = {"p": ((h & 0xff80) ^ 0x8000) - 0x8000, "i": min(h & 0x7f, 88)}
            pos += 2
            for k in range(32):
                out[c][2 * k] = ima_nib(s, bts[pos] & 15)
                out[c][2 * k + 1] = ima_nib(s, bts[pos] >> 4)
                pos += 1
    return np.array([[w(v << 16) for v in row] for row in out], np.int32), 0
