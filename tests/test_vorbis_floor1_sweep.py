"""Floor 1 on the device, swept: the two f32 closed forms of symphonia_amd/csrc/vorbis.hip -- render_line's
`trunc(f32(t) * slope + half)` and render_point's `trunc(f32(dy) * ratio + copysign(half, dy))` -- against plain integers, for
every segment length and every height difference a block can hold (tests/cpp/floor1_division_check.c proves the same
expressions on the host; here they go through the device's division, v_trunc_f32 and v_cvt_pk_u8_f32).

Section 1, segments: two-post floors xs = [0, X], multiplier 1 -- one segment (0, y0) -> (X, y1) and a flat tail -- with one
block for every dy in -255 .. 255; the expectation is  y(t) = y0 + sign(dy) * ((|dy| * t) // X)  below min(X, n), y1 from X on.
Section 2, posts: three-post floors xs = [0, A, x] whose third post is coded (val = 2), so that its height `predicted +- ...`
is a byte of the curve; the expectation is helpers.floor1_spec_model for the whole curve.
Every comparison is bit-equal; the byte form (what the product runs) takes everything, aligned and -- every 16th floor -- at
block starts 12 bytes off a 16-byte boundary between poisoned gaps; the f32 form takes every 16th floor.
The expectations never come from the library: test_models_agree_* (CPU) holds the spec model, its closed line form and the
oracle against each other on a thinned set of the same inputs before any of them judges a kernel."""
import numpy as np
import pytest

import oracle
from emu_lib import emu_ctx  # noqa: F401
from helpers import bit_equal, floor1_spec_model
from symphonia_amd import VorbisDsp
from test_vorbis_floor_y import db_table

POISON = 0xA5
LONG_X = (4097, 4111, 6000, 8191, 8192, 12289, 17018, 17019, 17020, 32767, 32768, 65535)
WIDE_A = (4097, 17019, 65535)


def block_n(X):
    return 4096 if X > 4096 else max(16, (X + 15) // 16 * 16)


def dy_rows():
    """(y0, y1) for dy = -255 .. 255: (0, dy) upwards, (255, 255 + dy) downwards"""
    dy = np.arange(-255, 256)
    y0 = np.where(dy >= 0, 0, 255)
    return np.stack([y0, y0 + dy], axis=1).astype(np.uint32)


def high_rows():
    """64 (y0, y1) with values up to 511 (beyond every range; |y1 - y0| never above 511): the four corners first"""
    rng = np.random.default_rng(511)
    rows = rng.integers(0, 512, size=(64, 2))
    rows[:4] = ((0, 511), (511, 0), (511, 1), (256, 511))
    rows[4:12, 0] = 511
    rows[12:20, 1] = 511
    return rows.astype(np.uint32)


def post_rows(high=True):
    """section 2's blocks: posts 0 and 1 from dy_rows() (+ high_rows()), post 2 coded with val = 2"""
    r = np.concatenate([dy_rows(), high_rows()]) if high else dy_rows()
    return np.concatenate([r, np.full((len(r), 1), 2, np.uint32)], axis=1)


class Numpy:
    xp = np

    @staticmethod
    def dev(a):
        return a

    @staticmethod
    def full(size, value, dtype):
        return np.full(size, value, dtype)

    @staticmethod
    def i64(a):
        return np.asarray(a).astype(np.int64)

    @staticmethod
    def counts(items):
        return [int(v) for v in items]

    @staticmethod
    def bits(a):
        return a.view(np.int32)


class Torch:
    def __init__(self):
        import torch
        self.xp = torch

    def dev(self, a):
        return self.xp.from_numpy(np.ascontiguousarray(a)).cuda()

    def full(self, size, value, dtype):
        return self.xp.full((size,), value, dtype=getattr(self.xp, np.dtype(dtype).name), device="cuda")

    def i64(self, a):
        return self.xp.from_numpy(np.asarray(a).astype(np.int64)).cuda()

    def counts(self, items):
        return self.xp.stack(list(items)).cpu().tolist() if items else []

    def bits(self, a):
        return a.view(self.xp.int32)


class Sweep:
    """Runs floors through the entry points and keeps ONE mismatch count per run on the array library's side; `finish` brings the counts
    back (one transfer) and, for the first run that differs, re-derives the first differing (block, line)."""

    def __init__(self, ctx, lib):
        self.v, self.lib, self.xp = VorbisDsp(ctx, 8, 11), lib, lib.xp
        self.db = lib.dev(db_table())
        self.runs, self.bad = [], []

    def segment_want(self, X, n, rows64):
        xp = self.xp
        t = xp.arange(n)[None, :] if xp is np else xp.arange(n, device="cuda")[None, :]
        y0, y1 = rows64[:, 0:1], rows64[:, 1:2]
        dy = y1 - y0
        sign = (dy >= 0) * 2 - 1
        return xp.where(t < X, y0 + sign * ((abs(dy) * t) // X), y1 + 0 * t)  # int64 [count, n]

    def run(self, label, xs, mult, n, d_ys, want, form, detail=False):
        """form: "bytes" (aligned, block b at b * n), "bytes+12" (block b at b * (n + 16) + 12 between poison) or "f32".  `want`: the
        expected table indices [count, n] on the array library's side."""
        xp, count = self.xp, int(d_ys.shape[0])
        if form == "f32":
            out = self.lib.full(count * n, 0.0, np.float32).reshape(count, n)
            self.v.floor1(xs, mult, d_ys, n, out, count)
            bad = self.lib.bits(out) != self.lib.bits(self.db[want if xp is np else want.long()])
        elif form == "bytes":
            plane = self.lib.full(count * n, POISON, np.uint8)
            self.v.floor1(xs, mult, d_ys, n, None, count, y_plane=plane)
            bad = plane.reshape(count, n) != want
        else:
            pitch = n + 16
            plane = self.lib.full(count * pitch + 32, POISON, np.uint8)
            offs = self.lib.dev((np.arange(count, dtype=np.uint32) * np.uint32(pitch) + np.uint32(12)))
            self.v.floor1(xs, mult, d_ys, n, None, count, y_plane=plane, line_offsets=offs)
            rows = plane[:count * pitch].reshape(count, pitch)
            bad = rows[:, 12:12 + n] != want
            gaps = (rows[:, :12] != POISON).sum() + (rows[:, 12 + n:] != POISON).sum() + (plane[count * pitch:] != POISON).sum()
            if detail:
                assert int(gaps) == 0, "%s: bytes outside the blocks were written" % (label,)
            self.bad.append(gaps)
            self.runs.append((label, None))
        if detail:
            return bad
        self.bad.append(bad.sum())
        self.runs.append((label, lambda: self.run(label, xs, mult, n, d_ys, want, form, detail=True)))

    def finish(self, describe):
        counts = self.lib.counts(self.bad)
        self.bad = []
        runs, self.runs = self.runs, []
        for (label, again), c in zip(runs, counts):
            if c:
                assert again is not None, "%s: %d bytes outside the blocks were written" % (label, c)
                bad = again()
                b, t = [int(v) for v in (np.argwhere(bad) if self.xp is np else bad.nonzero().cpu().numpy())[0]]
                raise AssertionError("%s: %d lines differ, first at %s" % (label, c, describe(label, b, t)))


# ---- section 1: segments -------------------------------------------------------------------------------------------------------

def check_segments(ctx, lib, Xs, rows_of, every=16):
    """rows_of(X) -> indices into dy_rows() (all 511 on the device); `every`: the unaligned byte form and the f32 form take the
    X that are multiples of it, the f32 form the long X as well"""
    s = Sweep(ctx, lib)
    all_rows = dy_rows()
    held = None  # the rows on the library's side, sent again only when they change (on the device every X takes all 511)
    for X in Xs:
        idx = rows_of(X)
        if held is None or not np.array_equal(held[0], idx):
            held = (idx, lib.dev(all_rows[idx]), lib.i64(all_rows[idx]))
        _, d_ys, rows64 = held
        n = block_n(X)
        want = s.segment_want(X, n, rows64)
        label = (X,)
        s.run(label + ("bytes",), [0, X], 1, n, d_ys, want, "bytes")
        if X % every == 0:
            s.run(label + ("bytes+12",), [0, X], 1, n, d_ys, want, "bytes+12")
        if X % every == 0 or X > 4096:
            s.run(label + ("f32",), [0, X], 1, n, d_ys, want, "f32")

    def describe(label, b, t):
        X, form = label[0], label[-1]
        return "(X, dy, t) = (%d, %d, %d), %s" % (X, int(rows_of(X)[b]) - 255, t, form)
    s.finish(describe)


EMU_X = sorted(set(range(1, 65)) | set(range(64 + 61, 4097, 61)) | set(LONG_X))


def emu_rows(X):
    """64 of the 511 dy per X, every 8th starting at X: any eight consecutive X cover all of them (8 * 64 = 511 + 1)"""
    return (np.arange(64) * 8 + X) % 511


def test_emu_floor1_segment_sweep(emu_ctx):
    check_segments(emu_ctx, Numpy, EMU_X, emu_rows)
    seen = np.zeros(511, bool)
    for X in EMU_X:
        seen[emu_rows(X)] = True
    assert seen.all()


def test_models_agree_on_segments():
    """CPU only.  The thinning: the emulation twin's X (1 .. 64, every 61st above, the long ones) with its 64 cyclic dy per X: on those,
    the line formula of section 1 == floor1_spec_model (the recurrence and its closed form) and dB[model] == the oracle, bit for bit."""
    s = Sweep.__new__(Sweep)
    s.xp = np
    db, rows = db_table(), dy_rows()
    for X in EMU_X:
        r, n = rows[emu_rows(X)], block_n(X)
        want = s.segment_want(X, n, r.astype(np.int64))
        model = floor1_spec_model([0, X], r, 1, n)
        assert np.array_equal(model, want) and np.array_equal(floor1_spec_model([0, X], r, 1, n, lines="closed"), want), X
        assert bit_equal(db[model], np.stack([oracle.vorbis_floor1([0, X], y, 1, n) for y in r])), X


# ---- section 2: posts ----------------------------------------------------------------------------------------------------------

def small_pairs():
    return [(A, x, 80 if A == 64 else 64) for A in range(2, 65) for x in range(1, A)]


def big_pairs(A, step=1):
    return [(A, x, 4096) for x in range(1, A, step)]


def wide_pairs(A):
    """256 values of x below 4096, one in every run of 16 lines"""
    return [(A, 16 * i + 1 + (5 * i) % 15, 4096) for i in range(256)]


def check_posts(ctx, lib, pairs, f32_every=16):
    s = Sweep(ctx, lib)
    rows, low = post_rows(), post_rows(high=False)
    d_rows, d_low = lib.dev(rows), lib.dev(low)
    m_rows, m_low = lib.i64(rows), lib.i64(low)
    for k, (A, x, n) in enumerate(pairs):
        xs = [0, A, x]
        want = floor1_spec_model(xs, m_rows, 1, n, lines="closed")
        s.run((A, x, 1, "bytes"), xs, 1, n, d_rows, want, "bytes")
        if k % f32_every == 0:
            s.run((A, x, 1, "bytes+12"), xs, 1, n, d_rows, want, "bytes+12")
            s.run((A, x, 1, "f32"), xs, 1, n, d_rows, want, "f32")
            # y up to 255 whatever the multiplier (what symaccel_vorbis_floor1_status_device lets through): the f32 entry point
            mult = 2 + (k // f32_every) % 3
            s.run((A, x, mult, "f32"), xs, mult, n, d_low, floor1_spec_model(xs, m_low, mult, n, lines="closed"), "f32")

    def describe(label, b, t):
        A, x, mult, form = label
        r = rows[b]
        return "(A, x, y0, y1, t) = (%d, %d, %d, %d, %d), multiplier %d, %s" % (A, x, r[0], r[1], t, mult, form)
    s.finish(describe)


# (the emulation runs a workgroup in ~10 ms whatever it renders: the twins are cut into cases of under 20 s, interleaved so that every
# case sees the whole range of A and x)
@pytest.mark.parametrize("part", range(8))
def test_emu_floor1_post_sweep_small(emu_ctx, part):
    check_posts(emu_ctx, Numpy, small_pairs()[part::8])


@pytest.mark.parametrize("A", (4096, 4093))
@pytest.mark.parametrize("part", range(2))
def test_emu_floor1_post_sweep_4096(emu_ctx, A, part):
    """every 64th x of the two longest closed-form spans"""
    check_posts(emu_ctx, Numpy, big_pairs(A, 64)[part::2])


@pytest.mark.parametrize("A", WIDE_A)
@pytest.mark.parametrize("part", range(6))
def test_emu_floor1_post_sweep_wide(emu_ctx, A, part):
    """the wide setups (integer render_point), all 256 x each"""
    check_posts(emu_ctx, Numpy, wide_pairs(A)[part::6])


def test_models_agree_on_posts():
    """CPU only.  The thinning: every (A, x) of A = 2 .. 64 with 36 of the 575 blocks (cyclically, all of them over 16 floors); every 256th
    x of A = 4096 and 4093 and every 32nd of the wide floors' 256 with all blocks.  On those: the recurrence == the closed line form, and
    dB[model] == the oracle, bit for bit; with y beyond the range (multipliers 2 .. 4) on every 16th."""
    db, rows, low = db_table(), post_rows(), post_rows(high=False)
    assert rows[:, :2].max() == 511 and abs(rows[:, 0].astype(int) - rows[:, 1].astype(int)).max() == 511
    thinned = [(p, (np.arange(36) * 16 + k) % len(rows)) for k, p in enumerate(small_pairs())]
    for A in (4096, 4093):
        thinned += [(p, np.arange(len(rows))) for p in big_pairs(A, 256)]
    for A in WIDE_A:
        thinned += [(p, np.arange(len(rows))) for p in wide_pairs(A)[::32]]
    for k, ((A, x, n), idx) in enumerate(thinned):
        cases = [(1, rows[idx])] + ([(2 + (k // 16) % 3, low[idx[idx < len(low)]])] if k % 16 == 0 else [])
        for mult, r in cases:
            xs = [0, A, x]
            model = floor1_spec_model(xs, r, mult, n)
            assert np.array_equal(model, floor1_spec_model(xs, r, mult, n, lines="closed")), (A, x, mult)
            assert bit_equal(db[model], np.stack([oracle.vorbis_floor1(xs, y, mult, n) for y in r])), (A, x, mult)


def test_setup_refuses_what_the_reference_cannot_render(emu_ctx):
    """the sweeps drop no case: what they leave out is what the reference itself cannot render -- a repeated x (render_line divides by
    x1 - x0, floor.rs:785-790) -- and that is refused before anything is written"""
    from symphonia_amd import SymaccelError
    plane = np.full(3 * 64, POISON, np.uint8)
    for xs in ([0, 64, 64], [0, 64, 0], [0, 0]):
        with pytest.raises(SymaccelError):
            VorbisDsp(emu_ctx, 8, 11).floor1(xs, 1, post_rows()[:3, :len(xs)].copy(), 64, None, 3, y_plane=plane)
    assert np.all(plane == POISON)


# ---- the same on the MI355X ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from symphonia_amd import Context
    ctx = Context(0)
    ctx.use_torch_stream()
    yield ctx, Torch()
    torch.cuda.synchronize()
    ctx.close()


ALL_ROWS = np.arange(511)


@pytest.mark.gpu
@pytest.mark.parametrize("first", range(1, 4097, 512))
def test_gpu_floor1_segment_sweep(gpu, first):
    """every X of a slice of 512 x every dy, on the device (the expectation in torch int64 there; one count per run comes back).
    Measured on the MI355X, seconds per slice (pytest's call duration, which ends with the transfer of the counts): 0.79 for the
    first one, which pays the first launches of the module, then 0.11, 0.12, 0.12, 0.11, 0.12, 0.15, 0.15; the long X together
    0.01.  (Section 2 there: A = 2 .. 64 1.6 s, a quarter of A = 4096 / 4093 0.8 - 1.0 s, a wide A 0.2 s.)"""
    check_segments(*gpu, range(first, first + 512), lambda X: ALL_ROWS)


@pytest.mark.gpu
def test_gpu_floor1_segment_sweep_long(gpu):
    check_segments(*gpu, LONG_X, lambda X: ALL_ROWS)


@pytest.mark.gpu
def test_gpu_floor1_post_sweep_small(gpu):
    check_posts(*gpu, small_pairs())


@pytest.mark.gpu
@pytest.mark.parametrize("A", (4096, 4093))
@pytest.mark.parametrize("part", range(4))
def test_gpu_floor1_post_sweep_4096(gpu, A, part):
    """every x below A, a quarter of them per case"""
    pairs = big_pairs(A)
    check_posts(*gpu, pairs[part * 1024:(part + 1) * 1024])


@pytest.mark.gpu
@pytest.mark.parametrize("A", WIDE_A)
def test_gpu_floor1_post_sweep_wide(gpu, A):
    check_posts(*gpu, wide_pairs(A))
