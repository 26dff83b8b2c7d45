"""TEST ONLY.  A small ADPCM encoder: int16 PCM -> the blocks symphonia-codec-adpcm's decode_mono / decode_stereo read (MS, IMA WAV,
IMA QT; mono and stereo).  It is no product code and aims at no quality target: it makes valid, varied packets whose decoded PCM tracks
a synthetic signal, so that the fixture's blocks exercise the recurrences the way real files do (steps that grow and shrink, both signs,
occasional clamps) -- what they decode to is decided by the reference under the interpreter, never by this file."""
import numpy as np

from adpcm_ref import IMA_INDEX, IMA_STEP, MS_ADAPT, MS_C1, MS_C2


def signal(seed, channels, frames, level=0.6):
    """int16[channels, frames]: two sines with a slow envelope plus noise, a loud burst in the middle (the burst drives the step up and
    clamps a few samples)"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)
    out = []
    for c in range(channels):
        x = np.sin(2 * np.pi * t * (0.011 + 0.004 * c)) * 0.6 + np.sin(2 * np.pi * t * 0.173 + c) * 0.3
        x *= 0.35 + 0.65 * np.abs(np.sin(2 * np.pi * t / max(frames, 1) * 1.5))
        x = x * level + rng.standard_normal(frames) * 0.02
        x[frames // 2:frames // 2 + 24] += (-1) ** c * 0.9
        out.append(np.clip(np.round(x * 32767), -32768, 32767))
    return np.array(out, np.int16)


def _clamp16(v):
    return max(-32768, min(32767, v))


def _tdiv256(v):
    return -((-v) // 256) if v < 0 else v // 256


class _Ima:
    def __init__(self, pred=0, idx=0):
        self.pred, self.idx = pred, idx

    def encode(self, s):
        step = int(IMA_STEP[self.idx])
        diff = int(s) - self.pred
        n = 0
        if diff < 0:
            n, diff = 8, -diff
        n |= min(7, (diff * 4) // step)
        d = ((2 * (n & 7) + 1) * step) >> 3
        self.pred = _clamp16(self.pred - d if n & 8 else self.pred + d)
        self.idx = max(0, min(88, self.idx + int(IMA_INDEX[n])))
        return n


def encode_ima_wav(pcm, fpb):
    """pcm int16[channels, n * fpb] -> uint8[n, block bytes]; mono: fpb odd, stereo: (fpb - 1) % 8 == 0"""
    ch, total = pcm.shape
    st = [_Ima() for _ in range(ch)]
    blocks = []
    for b0 in range(0, total - fpb + 1, fpb):
        x = pcm[:, b0:b0 + fpb]
        out = []
        for c in range(ch):
            st[c].pred = int(x[c, 0])
            out += [int(x[c, 0]) & 0xff, (int(x[c, 0]) >> 8) & 0xff, st[c].idx, 0]
        if ch == 1:
            for k in range((fpb - 1) // 2):
                lo = st[0].encode(x[0, 1 + 2 * k])
                out.append(lo | st[0].encode(x[0, 2 + 2 * k]) << 4)
        else:
            for g in range((fpb - 1) // 8):
                for c in range(2):
                    for j in range(4):
                        lo = st[c].encode(x[c, 1 + 8 * g + 2 * j])
                        out.append(lo | st[c].encode(x[c, 2 + 8 * g + 2 * j]) << 4)
        blocks.append(out)
    return np.array(blocks, np.uint8)


def encode_ima_qt(pcm):
    """pcm int16[channels, n * 64] -> uint8[n, 34 * channels]"""
    ch, total = pcm.shape
    st = [_Ima(int(pcm[c, 0]) if total else 0) for c in range(ch)]
    blocks = []
    for b0 in range(0, total - 63, 64):
        out = []
        for c in range(ch):
            h = (st[c].pred & 0xff80) | st[c].idx
            st[c].pred = ((h & 0xff80) ^ 0x8000) - 0x8000
            out += [h >> 8, h & 0xff]
            for k in range(32):
                lo = st[c].encode(pcm[c, b0 + 2 * k])
                out.append(lo | st[c].encode(pcm[c, b0 + 2 * k + 1]) << 4)
        blocks.append(out)
    return np.array(blocks, np.uint8)


class _Ms:
    def __init__(self, pi, s2, s1):
        self.c1, self.c2, self.s1, self.s2 = int(MS_C1[pi]), int(MS_C2[pi]), int(s1), int(s2)
        self.delta = max(16, abs(self.s1 - self.s2) // 3)

    def encode(self, s):
        lin = _tdiv256(self.s1 * self.c1 + self.s2 * self.c2)
        q = max(-8, min(7, int(round((int(s) - lin) / self.delta))))
        n = q & 15
        self.s2, self.s1 = self.s1, _clamp16(lin + q * self.delta)
        self.delta = max(16, _tdiv256(int(MS_ADAPT[n]) * self.delta))
        return n


def encode_ms(pcm, fpb):
    """pcm int16[channels, n * fpb] -> uint8[n, block bytes]; mono: fpb even; the block predictor cycles through all seven"""
    ch, total = pcm.shape
    blocks = []
    for bi, b0 in enumerate(range(0, total - fpb + 1, fpb)):
        x = pcm[:, b0:b0 + fpb]
        pis = [(bi + 3 * c) % 7 for c in range(ch)]
        st = [_Ms(pis[c], x[c, 0], x[c, 1]) for c in range(ch)]
        le = lambda v: [int(v) & 0xff, (int(v) >> 8) & 0xff]
        out = list(pis)
        for field in ("delta", "s1", "s2"):
            for c in range(ch):
                out += le(getattr(st[c], field))
        if ch == 1:
            for k in range(1, fpb // 2):
                hi = st[0].encode(x[0, 2 * k])
                out.append(hi << 4 | st[0].encode(x[0, 2 * k + 1]))
        else:
            for f in range(2, fpb):
                hi = st[0].encode(x[0, f])
                out.append(hi << 4 | st[1].encode(x[1, f]))
        blocks.append(out)
    return np.array(blocks, np.uint8)
