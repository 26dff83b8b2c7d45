"""TEST ONLY.  Writes MPEG audio Layer I and Layer II frames (ISO/IEC 11172-3 2.4.1-2.4.2, 13818-3 2.4) field by field, and gives the
same fields in the form symaccel_mpa12_decode takes them: 16-bit sample codes [channel][sub-band][sample] plus one record per
channel-packet.  The tables are the standard's (11172-3 Tables 3-B.2a-d, 3-B.4; 13818-3 Table B.1), written here from the standard;
nothing in this file decodes."""
import numpy as np

L1_RATES = {"1": [0, 32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 416, 448],
            "2": [0, 32, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 224, 256]}
L2_RATES = {"1": [0, 32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384],
            "2": [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160]}
SAMPLE_RATES = {"1": [44100, 48000, 32000], "2": [22050, 24000, 16000], "2.5": [11025, 12000, 8000]}
STEREO, JOINT, DUAL, MONO = 0, 1, 2, 3

# Table 3-B.4: (grouped, bits of a sample or of a grouped codeword, levels), in the order of increasing levels
CLASSES = [(True, 5, 3), (True, 7, 5), (False, 3, 7), (True, 10, 9)] + [(False, b, (1 << b) - 1) for b in range(4, 17)]
# Tables 3-B.2a-d / B.1: a sub-band's row = (nbal, class index for allocation values 1 .. 2^nbal - 1)
_R = {"A": (4, [0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]), "B": (4, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16]),
      "C": (3, [0, 1, 2, 3, 4, 5, 16]), "D": (2, [0, 1, 16]), "E": (4, [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]),
      "F": (3, [0, 1, 3, 4, 5, 6, 7]), "G": (4, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14]), "H": (2, [0, 1, 3])}
ALLOC_TABLES = {"a": [_R["A"]] * 3 + [_R["B"]] * 8 + [_R["C"]] * 12 + [_R["D"]] * 4,
                "b": [_R["A"]] * 3 + [_R["B"]] * 8 + [_R["C"]] * 12 + [_R["D"]] * 7,
                "c": [_R["E"]] * 2 + [_R["F"]] * 6,
                "d": [_R["E"]] * 2 + [_R["F"]] * 10,
                "m2": [_R["G"]] * 4 + [_R["F"]] * 7 + [_R["H"]] * 19}


def class_width(k):
    """bits of one raw sample of class k: a grouped codeword un-groups to samples below `levels`"""
    grouped, bits, levels = CLASSES[k]
    return (levels - 1).bit_length() if grouped else bits


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, bits):
        value, bits = int(value), int(bits)
        assert 0 <= value < (1 << bits), (value, bits)
        self.acc, self.n = (self.acc << bits) | value, self.n + bits

    def bytes(self, size):
        assert self.n <= 8 * size, "the fields need %d bits, the frame has %d" % (self.n, 8 * size)
        return (self.acc << (8 * size - self.n)).to_bytes(size, "big")


class Header:
    """version "1" / "2" / "2.5", layer 1 / 2, bit-rate index 1..14, sample-rate index 0..2, mode, mode extension (joint stereo: the
    bound is 4 * (1 + mode_ext)), CRC word present, padding"""

    def __init__(self, layer, version="1", rate_idx=14, sr_idx=0, mode=STEREO, mode_ext=0, crc=False, padding=False):
        self.layer, self.version, self.rate_idx, self.sr_idx, self.mode, self.mode_ext, self.crc, self.padding = layer, version, rate_idx, sr_idx, mode, mode_ext, crc, padding

    @property
    def channels(self):
        return 1 if self.mode == MONO else 2

    @property
    def bitrate(self):
        return 1000 * (L1_RATES if self.layer == 1 else L2_RATES)["1" if self.version == "1" else "2"][self.rate_idx]

    @property
    def sample_rate(self):
        return SAMPLE_RATES[self.version][self.sr_idx]

    @property
    def n_frames(self):
        return 12 if self.layer == 1 else 36

    def frame_bytes(self):
        if self.layer == 1:
            return 4 * (12 * self.bitrate // self.sample_rate + int(self.padding))
        return 144 * self.bitrate // self.sample_rate + int(self.padding)

    def word(self):
        v = {"1": 3, "2": 2, "2.5": 0}[self.version]
        return (0x7ff << 21) | (v << 19) | ((4 - self.layer) << 17) | (int(not self.crc) << 16) | (self.rate_idx << 12) | (self.sr_idx << 10) | \
            (int(self.padding) << 9) | (self.mode << 6) | (self.mode_ext << 4)

    def alloc_table(self):
        """Layer II: which of Tables 3-B.2a-d / B.1 the frame uses (11172-3 2.4.2.3)"""
        if self.version != "1":
            return "m2"
        per_channel = self.bitrate // self.channels
        if per_channel <= 48000:
            return "d" if self.sample_rate == 32000 else "c"
        if per_channel <= 80000:
            return "a"
        return "a" if self.sample_rate == 48000 else "b"

    def sblimit(self):
        return 32 if self.layer == 1 else len(ALLOC_TABLES[self.alloc_table()])

    def bound(self):
        return min(4 * (1 + self.mode_ext) if self.mode == JOINT else 32, self.sblimit())

    def start(self):
        bw = BitWriter()
        bw.put(self.word(), 32)
        if self.crc:
            bw.put(0xbeef, 16)  # (not checked by the decoders on this path)
        return bw


def layer1_frame(h, bits, scf, codes):
    """bits[ch][32] in {0, 2..15}, scf[ch][32] in 0..63, codes[ch][32][12]; sub-bands from the bound on take channel 0's bits and
    codes.  Returns the packet."""
    nch, bound = h.channels, h.bound()
    bw = h.start()
    for sb in range(32):
        for ch in range(nch if sb < bound else 1):
            assert bits[ch][sb] == 0 or 2 <= bits[ch][sb] <= 15
            bw.put(bits[ch][sb] - 1 if bits[ch][sb] else 0, 4)
    for sb in range(32):
        for ch in range(nch):
            if bits[ch if sb < bound else 0][sb]:
                bw.put(scf[ch][sb], 6)
    for s in range(12):
        for sb in range(32):
            for ch in range(nch if sb < bound else 1):
                if bits[ch][sb]:
                    bw.put(codes[ch][sb][s], bits[ch][sb])
    return bw.bytes(h.frame_bytes())


def layer1_inputs(h, bits, scf, codes):
    """(codes[ch][32][12] u16, rec[ch][64] u8) of the frame layer1_frame writes"""
    nch, bound = h.channels, h.bound()
    c, r = np.zeros((nch, 32, 12), np.uint16), np.zeros((nch, 64), np.uint8)
    for ch in range(nch):
        for sb in range(32):
            src = ch if sb < bound else 0
            r[ch, sb] = bits[src][sb]
            if bits[src][sb]:
                r[ch, 32 + sb] = scf[ch][sb]
                c[ch, sb] = codes[src][sb]
    return c, r


def scf_from_scfsi(scfsi, sent):
    """the three scale-factor indices of a sub-band from the pattern and the indices transmitted (11172-3 2.4.2.3)"""
    return {0: lambda s: [s[0], s[1], s[2]], 1: lambda s: [s[0], s[0], s[1]], 2: lambda s: [s[0], s[0], s[0]], 3: lambda s: [s[0], s[1], s[1]]}[scfsi](sent)


SCFSI_SENT = {0: 3, 1: 2, 2: 1, 3: 2}


def layer2_frame(h, alloc, scfsi, sent, values):
    """alloc[ch][sb] = the allocation value (0 .. 2^nbal - 1); scfsi[ch][sb] in 0..3; sent[ch][sb] = the SCFSI_SENT[scfsi] indices
    transmitted; values[ch][sb][12][3]: an ungrouped class's three raw samples per granule, a grouped class's CODEWORD in [..][0].
    Sub-bands from the bound on take channel 0's allocation and values."""
    nch, bound, rows = h.channels, h.bound(), ALLOC_TABLES[h.alloc_table()]
    bw = h.start()
    for sb, (nbal, _) in enumerate(rows):
        for ch in range(nch if sb < bound else 1):
            bw.put(alloc[ch][sb], nbal)
    live = lambda ch, sb: alloc[ch if sb < bound else 0][sb] != 0  # noqa: E731
    for sb in range(len(rows)):
        for ch in range(nch):
            if live(ch, sb):
                bw.put(scfsi[ch][sb], 2)
    for sb in range(len(rows)):
        for ch in range(nch):
            if live(ch, sb):
                assert len(sent[ch][sb]) == SCFSI_SENT[scfsi[ch][sb]]
                for v in sent[ch][sb]:
                    bw.put(v, 6)
    for gr in range(12):
        for sb, (_, classes) in enumerate(rows):
            for ch in range(nch if sb < bound else 1):
                if alloc[ch][sb]:
                    grouped, nbits, _ = CLASSES[classes[alloc[ch][sb] - 1]]
                    for i in range(1 if grouped else 3):
                        bw.put(values[ch][sb][gr][i], nbits)
    return bw.bytes(h.frame_bytes())


def layer2_inputs(h, alloc, scfsi, sent, values):
    """(codes[ch][32][36] u16, rec[ch][128] u8) of the frame layer2_frame writes: grouped codewords un-grouped (integer work that
    belongs with the bit reader), qclass = 1 + the class index"""
    nch, bound, rows = h.channels, h.bound(), ALLOC_TABLES[h.alloc_table()]
    c, r = np.zeros((nch, 32, 36), np.uint16), np.zeros((nch, 128), np.uint8)
    for ch in range(nch):
        for sb, (_, classes) in enumerate(rows):
            src = ch if sb < bound else 0
            if not alloc[src][sb]:
                continue
            k = classes[alloc[src][sb] - 1]
            grouped, _, levels = CLASSES[k]
            r[ch, sb] = 1 + k
            r[ch, 32 + sb:128:32] = scf_from_scfsi(scfsi[ch][sb], sent[ch][sb])
            for gr in range(12):
                v = values[src][sb][gr]
                if grouped:
                    w = int(v[0])
                    v = [w % levels, w // levels % levels, w // (levels * levels) % levels]
                c[ch, sb, 3 * gr:3 * gr + 3] = v
    return c, r


# ---- seeded frames that use what the formats allow and still fit the frame

def random_layer1(rng, h, widths=None, scf63=False):
    """a frame's fields: every bit width in `widths` (default 2..15) on some sub-band, as many sub-bands as the frame holds"""
    nch, bound, budget = h.channels, h.bound(), 8 * h.frame_bytes() - 32 - (16 if h.crc else 0)
    bits, scf = np.zeros((nch, 32), np.int64), rng.integers(0, 63, (nch, 32))
    budget -= 4 * (nch * bound + 32 - bound)
    order = [(sb, ch) for sb in rng.permutation(32) for ch in range(nch if sb < bound else 1)]
    todo = list(widths if widths is not None else range(2, 16))
    for sb, ch in order:
        w = todo.pop() if todo else int(rng.integers(2, 16))
        cost = 12 * w + 6 * (1 if sb < bound else nch)
        if cost <= budget:
            bits[ch, sb], budget = w, budget - cost
    if scf63:
        scf[:, ::5] = 63
    codes = np.zeros((nch, 32, 12), np.int64)
    for ch in range(nch):
        for sb in range(32):
            w = int(bits[ch, sb])
            if w:
                codes[ch, sb] = special_codes(rng, w, 12)
    return bits, scf, codes


def special_codes(rng, w, n):
    """n codes of width w: 0, all ones, the sign bit alone, the one that makes a + 1 == 0 (a = -1: the sign bit cleared, the rest
    set), then random ones"""
    first = [0, (1 << w) - 1, 1 << (w - 1), (1 << (w - 1)) - 1]
    out = rng.integers(0, 1 << w, n)
    k = min(n, len(first))
    out[:k] = first[:k]
    return rng.permutation(out)


def random_layer2(rng, h, want_classes=None):
    """a frame's fields: classes of `want_classes` first where a sub-band's row offers them, every scfsi, scale-factor index 63, a
    grouped codeword at the top of its field (above levels^3) among the values"""
    nch, bound, rows = h.channels, h.bound(), ALLOC_TABLES[h.alloc_table()]
    budget = 8 * h.frame_bytes() - 32 - (16 if h.crc else 0) - sum(nbal * (nch if sb < bound else 1) for sb, (nbal, _) in enumerate(rows))
    alloc, scfsi = np.zeros((nch, 32), np.int64), rng.integers(0, 4, (nch, 32))
    sent = [[None] * 32 for _ in range(nch)]
    values = np.zeros((nch, 32, 12, 3), np.int64)
    todo = list(want_classes if want_classes is not None else range(17))
    for sb in rng.permutation(len(rows)):
        for ch in range(nch if sb < bound else 1):
            classes = rows[sb][1]
            pick = next((k for k in todo if k in classes), None)
            k = pick if pick is not None else classes[int(rng.integers(0, len(classes)))]
            grouped, nbits, _ = CLASSES[k]
            chans = [ch] if sb < bound else list(range(nch))
            cost = 12 * nbits * (1 if grouped else 3) + sum(2 + 6 * SCFSI_SENT[int(scfsi[c, sb])] for c in chans)
            if cost > budget:
                continue
            budget -= cost
            if pick is not None:
                todo.remove(pick)
            alloc[ch, sb] = classes.index(k) + 1
            for g in range(12):
                if grouped:
                    values[ch, sb, g, 0] = rng.integers(0, 1 << nbits)
                else:
                    values[ch, sb, g] = special_codes(rng, nbits, 3)
            if grouped:
                values[ch, sb, 0, 0], values[ch, sb, 1, 0] = (1 << nbits) - 1, 0
    for ch in range(nch):
        for sb in range(len(rows)):
            s = rng.integers(0, 64, SCFSI_SENT[int(scfsi[ch, sb])])
            if (sb + ch) % 4 == 0:
                s[-1] = 63
            sent[ch][sb] = [int(x) for x in s]
    return alloc, scfsi, sent, values
