"""The verify forms of SYMACCEL_BATCH_FLAC_RESTORE: param = 0x200 | (nch - 1) << 12 (restore, then the STREAMINFO MD5 of
validate.rs:25-75 in the same launch; the planes come back as param = 0 leaves them) and 0x300 | out_shift | (nch - 1) << 12 (the
finishing MD5 kernel also leaves the planes decorrelated and left-justified, decoder.rs:231-242), and symaccel_flac_md5_finish_device
itself.  A submission is one stream's run of frames; its state plane holds one symaccel_md5_state per frame -- entry 0 goes in as the
starting state, entry f comes back as the state after frame f.

The expected digest is hashlib.md5 over the byte string test_flac_md5.pack() builds from the ORACLE's restored subframes (never from
the code under test); the expected planes are the oracle's restore, and for the finishing form numpy's decorrelation and wrapping `<<`.
Everything is bit-exact.  CPU emulation here, gpu-marked twins on the MI355X."""
import os

import numpy as np
import pytest

import oracle
from emu_lib import emu_ctx, emu_library  # noqa: F401
from symphonia_amd import (BATCH_FLAC_RESTORE, FLAC_MD5_FRAME_DTYPE, FLAC_MD5_JOB_DTYPE, MD5_STATE_DTYPE, Batcher, Context, SymaccelError, flac_desc,
                           flac_md5_finish_device, flac_md5_frames, md5_init, md5_update)
from test_flac_md5 import assert_state, decorrelate, pack

FLAC_VERBATIM, FLAC_FIXED, FLAC_LPC = 0, 1, 2
UNITS = 200
EDGE_BLOCKS = [1, 63, 64, 65, UNITS]


@pytest.fixture(scope="module")
def gpu_ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on an MI355X (there is no CPU path)")
    ctx = Context(0)
    yield ctx
    ctx.close()


def vparam(nch, finish=False, shift=0):
    return (0x300 | shift if finish else 0x200) | (nch - 1) << 12


def shl(v, shift):
    """the wrapping `<< shift` of decoder.rs:239-242 on i32"""
    return ((np.asarray(v, np.int64) & 0xffffffff) << shift & 0xffffffff).astype(np.uint32).view(np.int32)


class Stream:
    """One stream's run of frames: residual planes whose subframes are VERBATIM (samples of `bps` bits, about 2 % of them far outside:
    the truncation and the `<<` then differ from a mask), FIXED and LPC -- so the digest is right only if the restore ran first."""

    def __init__(self, seed, nch, nb, block_len, units=UNITS, widths=None, modes=None):
        rng = np.random.default_rng(seed)
        self.nch, self.nb, self.units = nch, nb, units
        self.block_len = np.asarray(block_len)
        nf = len(self.block_len)
        n = nf * nch
        bps = 8 * nb
        lim = 1 << (bps - 1)
        buf = rng.integers(-lim, lim, (n, units), dtype=np.int64)
        wild = rng.random(buf.shape) < 0.02
        buf[wild] = rng.integers(-(1 << 31), 1 << 31, int(wild.sum()))
        kind = rng.choice([FLAC_VERBATIM, FLAC_VERBATIM, FLAC_FIXED, FLAC_LPC], n).astype(np.uint8)
        order = np.where(kind == FLAC_FIXED, rng.integers(0, 5, n), rng.integers(1, 33, n)).astype(np.uint8)
        pred = kind != FLAC_VERBATIM  # residuals of a predictor: small, behind `order` warm-up samples
        buf[pred] = rng.integers(-64, 64, (int(pred.sum()), units))
        for f in range(nf):  # the words past a frame's block are zero padding
            buf[f * nch:(f + 1) * nch, self.block_len[f]:] = 0
        shift = rng.integers(0, 15, n).astype(np.uint8)
        wasted = np.where(rng.random(n) < 0.2, rng.integers(1, 4, n), 0).astype(np.uint8)
        self.buf = buf.astype(np.int32)
        self.desc = np.ascontiguousarray(flac_desc(kind, order, shift, wasted))
        self.coeffs = rng.integers(-(1 << 9), 1 << 9, (n, 32)).astype(np.int32)
        self.pair_mode = (np.asarray(modes) if modes is not None else rng.integers(0, 4, nf)) if nch == 2 else np.zeros(nf, np.int64)
        self.widths = np.full(nf, nb) if widths is None else np.asarray(widths)
        self.frames = flac_md5_frames(self.block_len, self.pair_mode, self.widths)
        self.restored = oracle.flac_restore(self.buf, oracle.flac_desc(kind, order, shift, wasted), self.coeffs)
        self.bytes = [pack(self.restored[f * nch:(f + 1) * nch], nch, self.block_len[f:f + 1], self.pair_mode[f:f + 1], int(self.widths[f])) for f in range(nf)]

    def finished(self, out_shift):
        """what the finishing form leaves: decorrelated and shifted up to the frame's block length, the restore's words beyond"""
        want = self.restored.copy()
        for f, n in enumerate(self.block_len):
            ch = [want[f * self.nch + c, :n].astype(np.int64) for c in range(self.nch)]
            if self.nch == 2 and self.pair_mode[f]:
                ch[0], ch[1] = decorrelate(int(self.pair_mode[f]), ch[0], ch[1])
            for c in range(self.nch):
                want[f * self.nch + c, :n] = shl(ch[c], out_shift)
        return want

    def states(self, lib, start=b""):
        st = np.zeros(len(self.block_len), MD5_STATE_DTYPE)
        first = md5_init(lib)
        md5_update(first, start, lib)
        st[0] = first[0]
        return st

    def submit(self, b, states, finish=False, shift=0, first=0, last=None):
        last = len(self.block_len) if last is None else last
        got = self.buf[first * self.nch:last * self.nch].copy()
        t = b.submit_flac_verify(got, self.desc[first * self.nch:last * self.nch], self.coeffs[first * self.nch:last * self.nch],
                                 np.ascontiguousarray(self.frames[first:last]), self.nch, states, finish=finish, out_shift=shift)
        return t, got

    def check_states(self, states, lib, start=b"", first=0):
        done = start + b"".join(self.bytes[:first])
        for k in range(len(states)):
            done += self.bytes[first + k]
            assert_state(states[k:k + 1], done, lib)


def check_layouts(ctx, nch, nb):
    """every channel count x width: the edge block lengths and random ones, all four pair modes, frames with a width of their own"""
    lib = ctx.lib
    rng = np.random.default_rng(nch * 10 + nb)
    bl = EDGE_BLOCKS + [int(x) for x in rng.integers(1, UNITS + 1, 3)]
    widths = [nb, nb, 1 + nb % 4, nb, nb, 1 + (nb + 1) % 4, nb, nb]
    s = Stream(100 * nch + nb, nch, nb, bl, widths=widths, modes=[0, 1, 2, 3, 2, 1, 3, 0])
    out_shift = 32 - 8 * nb
    b = Batcher(ctx, 0)
    st_plain, st_fin = s.states(lib, b"seed"), s.states(lib, b"seed")
    t0, got0 = s.submit(b, st_plain)
    t1, got1 = s.submit(b, st_fin, finish=True, shift=out_shift)
    plain = s.buf.copy()
    t2 = b.submit_flac_restore(plain, s.desc, s.coeffs)
    for t in (t0, t1, t2):
        b.collect(t)
    assert np.array_equal(plain, s.restored)
    assert np.array_equal(got0, plain), "0x200 must leave the planes as param = 0 does"
    assert np.array_equal(got1, s.finished(out_shift)), np.argwhere(got1 != s.finished(out_shift))[:5]
    s.check_states(st_plain, lib, b"seed")
    s.check_states(st_fin, lib, b"seed")
    assert b.stats()["failed_tickets"] == 0
    b.close()


def check_tail_carry(ctx):
    """frame byte counts that are no multiple of 64 (3 channels x 3 bytes x odd lengths): the tail carries across frames and across two
    successive tickets of one stream; the result equals one ticket holding all the frames"""
    lib = ctx.lib
    s = Stream(7, 3, 3, [5, 37, 1, 199, 64, 13, 77, 3, 101])
    b = Batcher(ctx, 0)
    whole = s.states(lib)
    tw, _ = s.submit(b, whole)
    b.collect(tw)
    s.check_states(whole, lib)
    assert all(int(x) % 64 for x in whole["len"])
    a = s.states(lib)[:4].copy()
    ta, _ = s.submit(b, a, last=4)
    b.collect(ta)
    c = np.zeros(5, MD5_STATE_DTYPE)
    c[0] = a[3]  # the second ticket starts where the first ended
    tc, _ = s.submit(b, c, first=4)
    b.collect(tc)
    s.check_states(a, lib)
    s.check_states(c, lib, first=4)
    assert c[4:].tobytes() == whole[8:].tobytes() and np.concatenate([a, c]).tobytes() == whole.tobytes()
    b.close()


def check_sharing(ctx):
    """two verified streams of different lengths share ONE launch; a plain submission of the same block size is a group of its own and
    is unaffected"""
    lib = ctx.lib
    s1, s2 = Stream(11, 2, 2, [UNITS] * 5 + [17]), Stream(12, 2, 2, [UNITS] * 8 + [99])
    p = Stream(13, 2, 2, [UNITS] * 3)
    b = Batcher(ctx, 0)
    st1, st2 = s1.states(lib), s2.states(lib, b"x" * 33)
    t1, g1 = s1.submit(b, st1)
    plain = p.buf.copy()
    tp = b.submit_flac_restore(plain, p.desc, p.coeffs)
    t2, g2 = s2.submit(b, st2)
    assert b.stats()["pending"] == 3
    for t in (t2, tp, t1):
        b.collect(t)
    st = b.stats()
    assert st["launches"] == 2 and st["max_chains_per_launch"] == (6 + 9) * 2 and st["failed_tickets"] == 0, st
    assert np.array_equal(plain, p.restored) and np.array_equal(g1, s1.restored) and np.array_equal(g2, s2.restored)
    s1.check_states(st1, lib)
    s2.check_states(st2, lib, b"x" * 33)
    b.close()


def check_chunks(ctx):
    """a group cut into chunks of whole submissions: one MD5 launch per chunk, every ticket its own digest"""
    lib = ctx.lib
    old = {k: os.environ.get(k) for k in ("SYMACCEL_BATCH_CHUNK_MIN_KB", "SYMACCEL_BATCH_CHUNKS")}
    os.environ["SYMACCEL_BATCH_CHUNK_MIN_KB"], os.environ["SYMACCEL_BATCH_CHUNKS"] = "64", "4"
    try:
        b = Batcher(ctx, 0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    streams = [Stream(20 + i, 3, 2, [UNITS] * (5 + i) + [1 + 31 * i]) for i in range(6)]
    subs = []
    for i, s in enumerate(streams):
        st = s.states(lib, bytes([i]) * (i * 11))
        subs.append((s, st, i) + s.submit(b, st, finish=True, shift=16))
    for s, st, i, t, got in subs:
        b.collect(t)
        s.check_states(st, lib, bytes([i]) * (i * 11))
        assert np.array_equal(got, s.finished(16))
    stt = b.stats()
    assert stt["launches"] == 1 and stt["chunks"] >= 2 and stt["failed_tickets"] == 0, stt
    b.close()


def check_row_pitch(ctx):
    """1024-sample blocks: the device plane's rows at symaccel_row_stride(1024) = 1152 words, and back to back (SYMACCEL_BATCH_ROW_PAD=0):
    the same digests and planes"""
    lib = ctx.lib
    assert lib.dll.symaccel_row_stride(1024) == 1152
    s = Stream(31, 2, 3, [1024, 1000, 1024, 65, 1024], units=1024)
    results = []
    for pad in (None, "0"):
        old = os.environ.get("SYMACCEL_BATCH_ROW_PAD")
        if pad is not None:
            os.environ["SYMACCEL_BATCH_ROW_PAD"] = pad
        try:
            b = Batcher(ctx, 0)
        finally:
            os.environ.pop("SYMACCEL_BATCH_ROW_PAD", None) if old is None else os.environ.__setitem__("SYMACCEL_BATCH_ROW_PAD", old)
        st0, st1 = s.states(lib), s.states(lib)
        t0, g0 = s.submit(b, st0)
        t1, g1 = s.submit(b, st1, finish=True, shift=8)
        b.collect(t0)
        b.collect(t1)
        s.check_states(st0, lib)
        s.check_states(st1, lib)
        assert np.array_equal(g0, s.restored) and np.array_equal(g1, s.finished(8))
        results.append((st0.tobytes(), st1.tobytes(), g0.tobytes(), g1.tobytes()))
        b.close()
    assert results[0] == results[1]


def hostile(kind, seed):
    """a stream whose description is refused, and the channel count of the group it rides in"""
    nch = 3 if kind == "mode_without_pair" else (1 if kind.startswith("mono_") else 2)
    s = Stream(seed, nch, 2, [UNITS, 50, 64, 1, 99])
    kind = kind[5:] if kind.startswith("mono_") else kind  # (the same refusals in a one-channel group: one state per CHAIN there)
    if kind == "block_len":
        s.frames["block_len"][2] = UNITS + 1
    elif kind == "pair_mode":
        s.frames["pair_mode"][4] = 4
    elif kind == "mode_without_pair":
        s.frames["pair_mode"][1] = 1
    elif kind == "width_0":
        s.frames["bytes_per_sample"][0] = 0
    elif kind == "width_5":
        s.frames["bytes_per_sample"][3] = 5
    elif kind == "restore_desc":
        s.desc["kind"][3], s.desc["order"][3] = FLAC_LPC, 33
    return s, nch


HOSTILE = ["block_len", "pair_mode", "mode_without_pair", "width_0", "width_5", "restore_desc", "mono_width_0", "mono_block_len", "mono_pair_mode", "mono_restore_desc"]


def check_bad_ticket(ctx, kind, finish):
    """a refused ticket between two good ones fails alone with INVALID_ARG, every state of it equal to its start; the neighbours are exact"""
    lib = ctx.lib
    bad, nch = hostile(kind, 40)
    left, right = Stream(41, nch, 2, [UNITS, 7, 64]), Stream(42, nch, 2, [65, UNITS, 3, 120])
    b = Batcher(ctx, 0)
    stl, stb, st_r = left.states(lib, b"left"), bad.states(lib, b"start of the bad one"), right.states(lib)
    tl, gl = left.submit(b, stl, finish=finish, shift=16 if finish else 0)
    tb, gb = bad.submit(b, stb, finish=finish, shift=16 if finish else 0)
    tr, gr = right.submit(b, st_r, finish=finish, shift=16 if finish else 0)
    b.collect(tl)
    with pytest.raises(SymaccelError) as e:
        b.collect(tb)
    assert e.value.status == -1
    b.collect(tr)
    for f in range(len(stb)):
        assert_state(stb[f:f + 1], b"start of the bad one", lib)
    assert np.array_equal(gb, bad.buf), "the buffer of a submission that failed alone is left as it was"
    left.check_states(stl, lib, b"left")
    right.check_states(st_r, lib)
    assert np.array_equal(gl, left.finished(16) if finish else left.restored) and np.array_equal(gr, right.finished(16) if finish else right.restored)
    st = b.stats()
    assert st["launches"] == 1 and st["failed_tickets"] == 1, st
    b.close()


def check_reserve_refusals(ctx):
    b = Batcher(ctx, 0)
    for param, n_chains in ((vparam(3), 7), (vparam(2), 3), (vparam(8), 12), (vparam(2) | 5, 4), (vparam(2) | 0x400, 4), (vparam(2) | 0x8000, 4),
                            (vparam(2) | 0x10000, 4), (vparam(2, True, 8) | 0x20, 4), (0x108 | 1 << 12, 4)):
        with pytest.raises(SymaccelError) as e:
            b.reserve(BATCH_FLAC_RESTORE, param, n_chains, UNITS)
        assert e.value.status == -1, hex(param)
    with pytest.raises(SymaccelError):
        b.reserve(BATCH_FLAC_RESTORE, vparam(2), 4, UNITS, out_format="s16", channels=2)
    t, slot = b.reserve(BATCH_FLAC_RESTORE, vparam(8, True, 31), 16, UNITS)  # every nch takes the finishing form
    assert slot.state_bytes[0] == 2 * MD5_STATE_DTYPE.itemsize and slot.input_bytes[3] == 2 * FLAC_MD5_FRAME_DTYPE.itemsize and slot.out == slot.input[0]
    b.release(t)
    b.close()


def check_finish_device(ctx, to_device, to_host):
    """symaccel_flac_md5_finish_device on a 3-frame, 2-channel job (and a neighbour that does not add up: nothing hashed, nothing written)"""
    lib = ctx.lib
    s = Stream(50, 2, 3, [UNITS, 65, 130], modes=[2, 1, 3])
    jobs = np.zeros(2, FLAC_MD5_JOB_DTYPE)
    states = np.concatenate([s.states(lib, b"abc")[:1]] * 2)
    bad_frames = s.frames.copy()
    bad_frames["pair_mode"][1] = 9
    d_rows = [to_device(s.restored), to_device(s.restored)]
    d_frames = [to_device(s.frames), to_device(bad_frames)]
    d_states, d_cps = to_device(states), to_device(np.zeros(6, MD5_STATE_DTYPE))
    for j in range(2):
        jobs[j]["rows"], jobs[j]["frames"] = d_rows[j][0], d_frames[j][0]
        jobs[j]["state"] = d_states[0] + j * MD5_STATE_DTYPE.itemsize
        jobs[j]["checkpoints"] = d_cps[0] + 3 * j * MD5_STATE_DTYPE.itemsize
        jobs[j]["row_pitch"], jobs[j]["n_frames"], jobs[j]["nch"], jobs[j]["bytes_per_sample"] = UNITS, 3, 2, 3
    d_jobs = to_device(jobs)
    flac_md5_finish_device(ctx, d_jobs[1], 8, 2)
    got_states = to_host(d_states, MD5_STATE_DTYPE, 2)
    cps = to_host(d_cps, MD5_STATE_DTYPE, 6)
    s.check_states(cps[:3], lib, b"abc")
    assert_state(got_states[:1], b"abc" + b"".join(s.bytes), lib)
    assert np.array_equal(to_host(d_rows[0], np.int32, s.restored.size).reshape(s.restored.shape), s.finished(8))
    for k in (3, 4, 5):
        assert_state(cps[k:k + 1], b"abc", lib)
    assert_state(got_states[1:], b"abc", lib)
    assert np.array_equal(to_host(d_rows[1], np.int32, s.restored.size).reshape(s.restored.shape), s.restored)


def host_device(a):
    a = np.ascontiguousarray(a).copy()
    return a.ctypes.data, a


def host_back(d, dtype, n):
    return d[1].view(np.uint8).ravel().view(dtype)[:n]


# ---- CPU emulation -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb", [1, 2, 3, 4])
@pytest.mark.parametrize("nch", [1, 2, 3, 8])
def test_emu_layouts(emu_ctx, nch, nb):
    check_layouts(emu_ctx, nch, nb)


def test_emu_tail_carries_across_frames_and_tickets(emu_ctx):
    check_tail_carry(emu_ctx)


def test_emu_verify_tickets_share_a_launch(emu_ctx):
    check_sharing(emu_ctx)


def test_emu_group_cut_into_chunks(emu_ctx):
    check_chunks(emu_ctx)


def test_emu_row_pitch(emu_ctx):
    check_row_pitch(emu_ctx)


@pytest.mark.parametrize("finish", [False, True])
@pytest.mark.parametrize("kind", HOSTILE)
def test_emu_bad_ticket_fails_alone(emu_ctx, kind, finish):
    check_bad_ticket(emu_ctx, kind, finish)


def test_emu_reserve_refusals(emu_ctx):
    check_reserve_refusals(emu_ctx)


def test_emu_finish_device(emu_ctx):
    check_finish_device(emu_ctx, host_device, host_back)


# ---- on the MI355X -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 2, 3, 4])
@pytest.mark.parametrize("nch", [1, 2, 3, 8])
def test_gpu_layouts(gpu_ctx, nch, nb):
    check_layouts(gpu_ctx, nch, nb)


@pytest.mark.gpu
def test_gpu_tail_carries_across_frames_and_tickets(gpu_ctx):
    check_tail_carry(gpu_ctx)


@pytest.mark.gpu
def test_gpu_verify_tickets_share_a_launch(gpu_ctx):
    check_sharing(gpu_ctx)


@pytest.mark.gpu
def test_gpu_group_cut_into_chunks(gpu_ctx):
    check_chunks(gpu_ctx)


@pytest.mark.gpu
def test_gpu_row_pitch(gpu_ctx):
    check_row_pitch(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("finish", [False, True])
@pytest.mark.parametrize("kind", HOSTILE)
def test_gpu_bad_ticket_fails_alone(gpu_ctx, kind, finish):
    check_bad_ticket(gpu_ctx, kind, finish)


@pytest.mark.gpu
def test_gpu_finish_device():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on an MI355X (there is no CPU path)")

    def to_device(a):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).ravel().copy()).cuda()
        return t.data_ptr(), t

    def to_host(d, dtype, n):
        torch.cuda.synchronize()
        return d[1].cpu().numpy().view(dtype)[:n]
    with Context(0) as ctx:  # (a context of its own: it joins torch's stream)
        ctx.use_torch_stream()
        check_finish_device(ctx, to_device, to_host)
