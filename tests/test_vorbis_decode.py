"""symaccel_vorbis_decode: the Vorbis tail host to host from what the packet decoder produces -- residue vectors, floor-1 posts,
the coupling steps of every block (lib.rs:250-331).  Expectation = the oracle chain in the reference's order: inverse coupling
(lib.rs:252-278, steps in order), floor curve (floor.rs:568-653), dot product (lib.rs:282-292; an unused floor is all zeros), then
DspChannel::synth (dsp.rs:68-126).  Several streams per batch, several floor configurations, chained coupling steps, channels whose
floor is unused with and without a coupled partner.  CPU emulation here, the MI355X under `-m gpu`."""
import numpy as np
import pytest

import oracle
from emu_lib import emu_ctx  # noqa: F401
from helpers import bit_equal, equal_mod_nan, floor1_spec_model, sprinkle_specials
from symphonia_amd import VORBIS_FLOOR1_DTYPE, SymaccelError, VorbisDsp


def make_floors(rng, bs0e, bs1e, n_floors, kind=None):
    """floor-1 configurations: the x list must fit the SHORT block too (floor1_X values are below the block's half size in a real
    setup; a post at or beyond n/2 just ends the rendering early, floor.rs:644-652).  kind: configuration 0 at a limit of the format --
    "posts65" (the largest post count: post 64 lives in `used_hi`), "two" (the smallest), "mult4" (the smallest range: y up to 63),
    "top15" (rangebits 15: an x list that reaches 1 << 15 whatever the block sizes; posts beyond both blocks, wide neighbour spans)"""
    floors = np.zeros(n_floors, VORBIS_FLOOR1_DTYPE)
    lists = []
    for f in range(n_floors):
        n_posts, mult = int(rng.integers(2, 30)), int(rng.integers(1, 5))
        top = 1 << (bs1e - 1)
        if f == 0 and kind is not None:
            n_posts = {"posts65": 65, "two": 2, "mult4": 20, "top15": 24}[kind]
            mult = 4 if kind == "mult4" else mult
            top = 1 << 15 if kind == "top15" else top
        xs = [0, top] + rng.permutation(np.arange(1, top))[:n_posts - 2].tolist()
        if f == 0 and kind == "top15":  # posts inside the short block, inside the long one only, and beyond both
            short, long_ = 1 << (bs0e - 1), 1 << (bs1e - 1)
            xs = [0, top] + [int(v) for v in np.concatenate([rng.choice(np.arange(1, short), 6, replace=False),
                                                              rng.choice(np.arange(short, long_), 6, replace=False),
                                                              rng.choice(np.arange(long_, top), n_posts - 14, replace=False)])]
        floors[f]["multiplier"], floors[f]["n_posts"] = mult, n_posts
        floors[f]["x_list"][:n_posts] = xs
        lists.append((xs, mult))
    return floors, lists


def special_block(s, b):
    """the blocks of stream s that carry non-finite residue: every fourth, so that the blocks between them stay finite (a block's
    spectrum reaches its own PCM and, through the overlap, the next block's)"""
    return b % 4 == 1


def case(seed, bs0e, bs1e, n_streams, cps, nb, n_floors=2, stride_pad=0, specials=False, floor_kind=None):
    """stride_pad: lines beyond the packed length in spec_stride (a multiple of 4: with 4, 8 or 12 the rows of the byte plane are not
    16-byte aligned).  specials: +-Inf, NaN, -0.0 and denormals in the residue of the special_block()s, whose coupling is then a chain of
    two steps through one channel (or none: plain channels, alternating) and whose last channel has no floor but a coupled partner in use."""
    rng = np.random.default_rng(seed)
    nch = n_streams * cps
    flags = np.repeat(rng.integers(0, 2, (n_streams, nb)).astype(np.uint8), cps, axis=0)
    prev = np.repeat(rng.integers(-1, 2, n_streams).astype(np.int32), cps)
    so, po = oracle.vorbis_layout(bs0e, bs1e, flags, prev)
    spec_stride = (int(so[:, -1].max() + 3) & ~3) + stride_pad
    pcm_stride = int(po[:, -1].max() + 3) & ~3
    residue = (rng.standard_normal((nch, spec_stride)) * np.exp2(rng.integers(-3, 6, (nch, 1)))).astype(np.float32)
    residue[rng.random(residue.shape) < 0.2] = 0.0
    residue[rng.random(residue.shape) < 0.02] *= -0.0
    overlap = rng.standard_normal((nch, 1 << (bs1e - 1))).astype(np.float32)
    floors, lists = make_floors(rng, bs0e, bs1e, n_floors, floor_kind)
    floor = rng.integers(0, n_floors, (nch, nb)).astype(np.uint8)
    floor[rng.random((nch, nb)) < 0.25] = 255
    if specials:
        for s in range(n_streams):
            for b in range(nb):
                if special_block(s, b):
                    floor[s * cps:(s + 1) * cps, b] = np.minimum(floor[s * cps:(s + 1) * cps, b], n_floors - 1)
                    if cps > 1:
                        floor[(s + 1) * cps - 1, b] = 255
    posts = np.zeros((nch, nb, 65), np.uint32)
    for c in range(nch):
        for b in range(nb):
            if floor[c, b] != 255:
                mult = lists[floor[c, b]][1]
                y = rng.integers(0, [256, 128, 86, 64][mult - 1], 65)
                y[rng.random(65) < 0.2] = 0
                if floor_kind == "posts65" and floor[c, b] == 0:
                    y[64] = 0 if b % 2 == 0 else max(1, int(y[64]))  # post 64 coded in the odd blocks only
                if floor_kind == "mult4" and floor[c, b] == 0:
                    y[rng.random(65) < 0.4] = 63  # the top of the range: 63 * 4 = 252, the clamp at 255 stays out of reach
                posts[c, b] = y
    steps, first = [], [0]
    for s in range(n_streams):
        for b in range(nb):
            for _ in range(int(rng.integers(0, 4)) if cps > 1 else 0):
                m, a = rng.choice(cps, 2, replace=False)
                if not (specials and special_block(s, b)):
                    steps.append((int(m), int(a)))
            if specials and special_block(s, b) and cps > 1 and (b // 4 + s) % 2 == 0:
                steps += [(0, 1), (1, cps - 1)] if cps > 2 else [(0, 1), (1, 0)]  # two steps through channel 1; the last channel has no floor
            first.append(len(steps))
    coupling = np.array(steps, np.uint8).reshape(-1, 2)
    first = np.array(first, np.uint32)
    if specials:
        for s in range(n_streams):
            for b in range(nb):
                if special_block(s, b):
                    lo, hi = so[s * cps, b], so[s * cps, b + 1]
                    for c in range(s * cps, (s + 1) * cps):
                        block = residue[c:c + 1, lo:hi]
                        sprinkle_specials(block, rng, [0], per_unit=6)
                        block[0, rng.integers(0, hi - lo, 6)] = np.array([-0.0, 1e-41, -1e-41] * 2, np.float32)
    # a do-not-decode channel (unused floor and, after the propagation of lib.rs:215-228, no coupled partner in use): zero residue
    for s in range(n_streams):
        for b in range(nb):
            lo, hi = first[s * nb + b], first[s * nb + b + 1]
            used = np.array([floor[s * cps + c, b] != 255 for c in range(cps)])
            dnd = ~used
            for m, a in coupling[lo:hi]:
                if dnd[m] != dnd[a]:
                    dnd[m] = dnd[a] = False
            for c in range(cps):
                if dnd[c]:
                    residue[s * cps + c, so[s * cps, b]:so[s * cps, b + 1]] = 0.0
    return flags, prev, residue, overlap, pcm_stride, floors, lists, floor, posts, coupling, first, so


def spectrum_of(cps, flags, residue, lists, floor, posts, coupling, first, so):
    nch, nb = flags.shape
    res = residue.copy()
    spectrum = np.zeros_like(res)
    for s in range(nch // cps):
        for b in range(nb):
            lo, hi = so[s * cps, b], so[s * cps, b + 1]
            for m, a in coupling[first[s * nb + b]:first[s * nb + b + 1]]:
                res[s * cps + m, lo:hi], res[s * cps + a, lo:hi] = oracle.vorbis_inverse_coupling(res[s * cps + m, lo:hi], res[s * cps + a, lo:hi])
            for c in range(s * cps, (s + 1) * cps):
                n2 = hi - lo
                if floor[c, b] == 255:
                    curve = np.zeros(n2, np.float32)
                else:
                    xs, mult = lists[floor[c, b]]
                    curve = oracle.vorbis_floor1(xs, posts[c, b, :len(xs)], mult, n2)
                spectrum[c, lo:hi] = oracle.vorbis_dot_product(curve, res[c, lo:hi])
    return spectrum


def expectation(bs0e, bs1e, cps, flags, prev, residue, overlap, pcm_stride, lists, floor, posts, coupling, first, so):
    spectrum = spectrum_of(cps, flags, residue, lists, floor, posts, coupling, first, so)
    return oracle.vorbis_synth(bs0e, bs1e, spectrum, flags, prev, overlap, pcm_stride)


def run(ctx, seed, bs0e, bs1e, n_streams, cps, nb, **kw):
    flags, prev, residue, overlap, pcm_stride, floors, lists, floor, posts, coupling, first, so = case(seed, bs0e, bs1e, n_streams, cps, nb, **kw)
    want = expectation(bs0e, bs1e, cps, flags, prev, residue, overlap, pcm_stride, lists, floor, posts, coupling, first, so)
    v = VorbisDsp(ctx, bs0e, bs1e)
    pf, ov = prev.copy(), overlap.copy()
    pcm = np.zeros((flags.shape[0], pcm_stride), np.float32)
    before = residue.copy()
    v.decode(residue, flags, floor, posts, floors, cps, coupling, first, pf, ov, pcm_stride, pcm)
    assert bit_equal(residue, before), "the caller's residue must not be touched"
    if kw.get("specials"):  # NaN exactly where the reference has one, every other value bit for bit
        assert equal_mod_nan(pcm, want[0]), (bs0e, bs1e, n_streams, cps, nb, kw)
        assert equal_mod_nan(ov, want[1]) and np.array_equal(pf, want[2])
        return
    assert bit_equal(pcm, want[0]), (bs0e, bs1e, n_streams, cps, nb, kw)
    assert bit_equal(ov, want[1]) and np.array_equal(pf, want[2])


CASES = [(8, 11, 2, 2, 7), (6, 9, 1, 3, 9), (7, 10, 3, 1, 5), (8, 8, 1, 2, 4), (9, 12, 1, 4, 5)]


@pytest.mark.parametrize("bs0e,bs1e,n_streams,cps,nb", CASES)
def test_emu_vorbis_decode(emu_ctx, bs0e, bs1e, n_streams, cps, nb):
    run(emu_ctx, 40 + bs0e + 16 * bs1e + nb, bs0e, bs1e, n_streams, cps, nb)


# What decode had not seen.  Rows of the byte plane that are not 16-byte aligned (spec_stride = the packed length + 4, + 8, + 12 lines: channel
# c's row starts c * spec_stride bytes into the plane, so 1024- and 2048-line blocks take render_bytes<4>'s four 4-byte stores); special values
# in the residue; floors at the limits of the format.
EDGE_CASES = [(8, 11, 2, 2, 7, dict(stride_pad=4)), (9, 12, 1, 4, 5, dict(stride_pad=12)), (7, 10, 3, 1, 5, dict(stride_pad=8)),
              (8, 12, 1, 3, 6, dict(stride_pad=4)),
              (8, 11, 2, 3, 9, dict(specials=True)), (7, 10, 1, 2, 9, dict(specials=True, stride_pad=4)), (6, 9, 2, 4, 6, dict(specials=True)),
              (8, 11, 2, 2, 7, dict(floor_kind="posts65")), (6, 9, 1, 3, 9, dict(floor_kind="two")), (7, 10, 2, 2, 6, dict(floor_kind="mult4")),
              (8, 11, 1, 2, 6, dict(floor_kind="top15", stride_pad=8))]
EDGE_IDS = ["-".join(str(v) for v in c[:5]) + "-" + "-".join("%s=%s" % kv for kv in c[5].items()) for c in EDGE_CASES]


def edge_seed(bs0e, bs1e, nb):
    return 240 + bs0e + 16 * bs1e + nb


@pytest.mark.parametrize("bs0e,bs1e,n_streams,cps,nb,kw", EDGE_CASES, ids=EDGE_IDS)
def test_emu_vorbis_decode_edges(emu_ctx, bs0e, bs1e, n_streams, cps, nb, kw):
    run(emu_ctx, edge_seed(bs0e, bs1e, nb), bs0e, bs1e, n_streams, cps, nb, **kw)


@pytest.mark.parametrize("bs0e,bs1e,n_streams,cps,nb,kw", EDGE_CASES, ids=EDGE_IDS)
def test_edge_cases_are_what_they_claim(bs0e, bs1e, n_streams, cps, nb, kw):
    """CPU only: the properties of the inputs and of the oracle's answer that make the edge cases edges"""
    flags, prev, residue, overlap, pcm_stride, floors, lists, floor, posts, coupling, first, so = case(edge_seed(bs0e, bs1e, nb), bs0e, bs1e,
                                                                                                        n_streams, cps, nb, **kw)
    spec_stride = residue.shape[1]
    # the curves of the expectation: the independent model of Vorbis I 7.2.4 through the dB table == the oracle
    table = oracle.vorbis_floor1_table()
    for c in range(flags.shape[0]):
        for b in range(nb):
            if floor[c, b] != 255:
                (xs, mult), n2 = lists[floor[c, b]], int(so[c, b + 1] - so[c, b])
                y = posts[c, b, :len(xs)]
                assert bit_equal(table[floor1_spec_model(xs, y, mult, n2)], oracle.vorbis_floor1(xs, y, mult, n2)), (c, b)
    if kw.get("stride_pad"):
        assert spec_stride % 4 == 0 and spec_stride % 16 == kw["stride_pad"]
        starts = {(c * spec_stride + so[c, b]) % 16 for c in range(flags.shape[0]) for b in range(nb) if floor[c, b] != 255 and flags[c, b]}
        assert starts - {0}, "no long block starts off a 16-byte boundary"
    if kw.get("specials"):
        spectrum = spectrum_of(cps, flags, residue, lists, floor, posts, coupling, first, so)
        pcm = oracle.vorbis_synth(bs0e, bs1e, spectrum, flags, prev, overlap, pcm_stride)[0]
        po = oracle.vorbis_layout(bs0e, bs1e, flags, prev)[1]
        assert np.isnan(pcm).any()
        for s in range(n_streams):
            rows = slice(s * cps, (s + 1) * cps)
            assert any(np.isfinite(pcm[rows, po[s * cps, b]:po[s * cps, b + 1]]).all() for b in range(nb) if po[s * cps, b + 1] > po[s * cps, b]), s
        killed = [spectrum[c, so[c, b]:so[c, b + 1]] for c in range(flags.shape[0]) for b in range(nb) if floor[c, b] == 255]
        assert any(((k == 0) & np.signbit(k)).any() for k in killed), "no -0.0 product in a channel without a floor"
        assert any(np.isnan(k).any() for k in killed), "no 0.0 * Inf in a channel without a floor"
        chained = [coupling[first[i]:first[i + 1]] for i in range(n_streams * nb)]
        assert any(len(c) == 2 and c[0][1] == c[1][0] for c in chained), "no chain of two steps through one channel"
    kind = kw.get("floor_kind")
    if kind == "posts65":
        assert floors[0]["n_posts"] == 65
        coded = {bool(posts[c, b, 64]) for c in range(flags.shape[0]) for b in range(nb) if floor[c, b] == 0}
        assert coded == {False, True}
    if kind == "two":
        assert floors[0]["n_posts"] == 2 and (floor == 0).any()
    if kind == "mult4":
        assert floors[0]["multiplier"] == 4 and posts[floor == 0].max() == 63
    if kind == "top15":
        xs = lists[0][0]
        assert max(xs) == 1 << 15 and (1 << (bs1e - 1)) == 1024 and (1 << (bs0e - 1)) == 128 and (floor == 0).any()


def check_coupling_dot_specials(ctx, to_dev, to_host):
    """the same special values through the device-pointer helpers: inverse coupling as a chain of two steps through channel 1
    (lib.rs:252-278) and the dot product with a curve that has zeros (lib.rs:289-291: 0.0 * Inf is NaN, 0.0 * -x is -0.0)"""
    rng = np.random.default_rng(77)
    v = VorbisDsp(ctx, 8, 11)
    n = 1000
    res = (rng.standard_normal((3, n)) * np.exp2(rng.integers(-3, 6, (3, 1)))).astype(np.float32)
    res[rng.random(res.shape) < 0.2] = 0.0
    sprinkle_specials(res, rng, [0, 1, 2, 0, 1, 2], per_unit=30)
    for c in range(3):
        res[c, rng.integers(0, n, 30)] = np.array([-0.0, 1e-41, -1e-41] * 10, np.float32)
    want = res.copy()
    for m, a in ((0, 1), (1, 2)):
        want[m], want[a] = oracle.vorbis_inverse_coupling(want[m], want[a])
    d = to_dev(res)
    v.inverse_coupling(d, n, [0, 1], [1, 2])
    got = to_host(d)
    assert np.isnan(want).any() and np.isinf(want).any() and equal_mod_nan(got, want)
    curve = oracle.vorbis_floor1_table()[rng.integers(0, 256, (3, n))]
    curve[rng.random(curve.shape) < 0.5] = 0.0
    want_dot = oracle.vorbis_dot_product(curve, want)
    d_curve = to_dev(curve)
    v.dot_product(d_curve, to_dev(want), 3 * n)
    assert ((want_dot == 0) & np.signbit(want_dot)).any() and np.isnan(want_dot).any() and equal_mod_nan(to_host(d_curve), want_dot)


def test_emu_coupling_dot_specials(emu_ctx):
    check_coupling_dot_specials(emu_ctx, lambda a: a, lambda a: a)


def test_emu_vorbis_decode_argument_checks(emu_ctx):
    flags, prev, residue, overlap, pcm_stride, floors, lists, floor, posts, coupling, first, so = case(3, 8, 11, 1, 2, 4)
    v = VorbisDsp(emu_ctx, 8, 11)
    pcm = np.zeros((2, pcm_stride), np.float32)
    args = lambda **kw: dict(dict(residue=residue, block_flag=flags, floor=floor, posts=posts, floors=floors, channels_per_stream=2,  # noqa: E731
                                  coupling=coupling, coupling_first=first, prev_flag=prev.copy(), overlap=overlap.copy(), pcm_stride=pcm_stride,
                                  pcm=pcm), **kw)
    bad_flags = flags.copy()
    bad_flags[1, 0] ^= 1  # the channels of a stream must share their block flags
    with pytest.raises(SymaccelError):
        v.decode(**args(block_flag=bad_flags))
    bad_floor = floor.copy()
    bad_floor[0, 0] = 7  # names no configuration
    with pytest.raises(SymaccelError):
        v.decode(**args(floor=bad_floor))
    bad_steps = np.array([[0, 0]], np.uint8)  # a channel coupled with itself (lib.rs:253)
    with pytest.raises(SymaccelError):
        v.decode(**args(coupling=bad_steps, coupling_first=np.array([0, 1, 1, 1, 1], np.uint32)))
    big = posts.copy()
    big[floor != 255] = 600  # outside the closed form's range: the caller renders such a block itself
    with pytest.raises(SymaccelError) as e:
        v.decode(**args(posts=big))
    assert e.value.status == -2


@pytest.mark.gpu
@pytest.mark.parametrize("bs0e,bs1e,n_streams,cps,nb", CASES + [(8, 11, 8, 8, 40), (10, 13, 2, 2, 9), (12, 13, 1, 2, 6)])
def test_gpu_vorbis_decode(bs0e, bs1e, n_streams, cps, nb):
    from symphonia_amd import Context
    ctx = Context(0)
    run(ctx, 140 + bs0e + 16 * bs1e + nb, bs0e, bs1e, n_streams, cps, nb)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bs0e,bs1e,n_streams,cps,nb,kw", EDGE_CASES, ids=EDGE_IDS)
def test_gpu_vorbis_decode_edges(bs0e, bs1e, n_streams, cps, nb, kw):
    from symphonia_amd import Context
    ctx = Context(0)
    run(ctx, edge_seed(bs0e, bs1e, nb), bs0e, bs1e, n_streams, cps, nb, **kw)
    ctx.close()


@pytest.mark.gpu
def test_gpu_coupling_dot_specials():
    import torch
    from symphonia_amd import Context
    ctx = Context(0)
    ctx.use_torch_stream()
    check_coupling_dot_specials(ctx, lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda(), lambda t: t.cpu().numpy())
    ctx.close()
