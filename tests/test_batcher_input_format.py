"""The batcher's widening gather (symaccel_batcher_reserve_io / _submit_io): plane 0 of a FLAC_RESTORE / ALAC_PREDICT submission handed
over as int16_t and sign-extended into the i32 device plane by the gather of the launch.

Every comparison is BIT-EQUAL, and the reference is the SAME submission sent wide (in_fmt = 0) through a batcher of its own; for one
shape per kind the reference is the oracle's restore / predict as well.  The planes hold words of the whole int16_t range, and -32768,
32767, -1 and 0 stand at the first words of every row (warm-up positions), at its last words (residual positions) and on both sides of
every piece boundary (4096 words of the destination) of a row and of the compact plane.  CPU emulation here, gpu-marked twins of the same
cases on the MI355X."""

import numpy as np
import pytest

import oracle
from emu_lib import emu_ctx, emu_library  # noqa: F401
from symphonia_amd import (BATCH_AAC_SYNTH, BATCH_ALAC_PREDICT, BATCH_FLAC_RESTORE, MD5_STATE_DTYPE, Batcher, Context, SymaccelError, alac_desc,
                           flac_desc, flac_md5_frames, md5_init)
from symphonia_amd.backend import FLAC_FIXED, FLAC_LPC, FLAC_VERBATIM
from test_batcher_output_format import view
from test_pcm_convert import BYTES

UNITS = [1, 3, 17, 100, 1024, 4096, 4608, 8192, 65535]
SPECIAL = np.array([-32768, 32767, -1, 0], np.int32)
PIECE = 4096  # words of the destination in one copy piece
POISON = 0xA5
GUARD = 0x5A


def plane(rng, n_chains, units):
    """words of the whole int16_t range; the four special words at the first and the last words of every row and around every piece
    boundary -- of a row (padded device rows go row by row) and of the compact plane (rows back to back go as one run)"""
    buf = rng.integers(-32768, 32768, (n_chains, units)).astype(np.int32)
    k = min(4, units)
    buf[:, :k] = SPECIAL[:k]
    buf[:, units - k:] = SPECIAL[4 - k:]
    for edge in range(PIECE, units - 1, PIECE):
        buf[:, edge - 2:edge + 2] = SPECIAL
    flat = buf.reshape(-1)
    for edge in range(PIECE, flat.size - 1, PIECE):
        flat[edge - 2:edge + 2] = SPECIAL
    return buf


def sub_flac(seed, n_chains, units, param=0, max_order=32):
    rng = np.random.default_rng(seed)
    buf = plane(rng, n_chains, units)
    kind = rng.integers(0, 3, n_chains).astype(np.uint8)
    order = np.minimum(np.where(kind == FLAC_FIXED, rng.integers(0, 5, n_chains), rng.integers(1, 33, n_chains)), min(units, max_order)).astype(np.uint8)
    kind[(kind == FLAC_LPC) & (order == 0)] = FLAC_VERBATIM
    shift = rng.integers(0, 16, n_chains).astype(np.uint8)
    wasted = np.where(rng.random(n_chains) < 0.2, rng.integers(1, 4, n_chains), 0).astype(np.uint8)
    coeffs = rng.integers(-(1 << 14), 1 << 14, (n_chains, 32)).astype(np.int32)
    s = dict(kind=BATCH_FLAC_RESTORE, param=param, n_chains=n_chains, units=units, ins=[buf, np.ascontiguousarray(flac_desc(kind, order, shift, wasted)), coeffs],
             states=[], channels=2, oracle=lambda: oracle.flac_restore(buf, oracle.flac_desc(kind, order, shift, wasted), coeffs))
    if (param & 0x300) == 0x100:
        s["ins"].append(rng.integers(0, 4, n_chains // 2).astype(np.uint8))
    return s


def sub_flac_verify(lib, seed, n_frames, units, param):
    """a verify form (nch = 2): the frame records behind the coefficients, one MD5 state per frame (entry 0 the starting state)"""
    rng = np.random.default_rng(seed)
    s = sub_flac(seed, 2 * n_frames, units, param)
    block_len = rng.integers(1, units + 1, n_frames)
    block_len[0] = units
    s["ins"].append(np.ascontiguousarray(flac_md5_frames(block_len, rng.integers(0, 4, n_frames), np.full(n_frames, 2))))
    st = np.zeros(n_frames, MD5_STATE_DTYPE)
    st[0] = md5_init(lib)[0]
    s["states"] = [st]
    return s


def sub_alac(seed, n_chains, units, param=0, max_order=31):
    rng = np.random.default_rng(seed)
    buf = plane(rng, n_chains, units)
    mode = rng.choice([0, 0, 0, 15], n_chains).astype(np.uint8)
    order = np.minimum(rng.choice([0, 1, 2, 3, 4, 8, 12, 16, 31], n_chains), max_order).astype(np.uint8)
    shift = rng.integers(0, 16, n_chains).astype(np.uint8)
    bps = rng.choice([16, 20, 24, 32], n_chains).astype(np.uint8)
    coeffs = rng.integers(-(1 << 15), 1 << 15, (n_chains, 32)).astype(np.int32)
    s = dict(kind=BATCH_ALAC_PREDICT, param=param, n_chains=n_chains, units=units, ins=[buf, np.ascontiguousarray(alac_desc(mode, order, shift, bps)), coeffs],
             states=[], channels=2, oracle=lambda: oracle.alac_predict(buf, oracle.alac_desc(mode, order, shift, bps), coeffs))
    if param == 0x100:
        s["ins"] += [rng.integers(-3, 4, n_chains // 2).astype(np.int32), rng.integers(0, 32, n_chains // 2).astype(np.uint8)]
    return s


MAKE = {"flac": sub_flac, "alac": sub_alac}


def run_group(ctx, subs, modes, poison=False):
    """the submissions through ONE batcher of their own, zero-copy form; modes[i] = (narrow, out_format, channels).  Per ticket: status, the
    valid output bytes, the state planes, input_bytes[0] and out_bytes at reserve(); and the batcher's statistics"""
    b = Batcher(ctx, 0)
    live = []
    for s, (narrow, fmt, ch) in zip(subs, modes):
        t, slot = b.reserve(s["kind"], s["param"], s["n_chains"], s["units"], out_format=fmt or 0, channels=ch, in_fmt="s16" if narrow else 0)
        assert slot.out == slot.input[0]
        for k, a in enumerate(s["ins"]):
            a = np.ascontiguousarray(a)
            if k == 0 and narrow:
                assert np.array_equal(a.astype(np.int16), a)
                a = a.astype(np.int16)
            dst = view(slot.input[k], slot.input_bytes[k])
            src = a.view(np.uint8).ravel()
            assert len(src) == len(dst), (k, len(src), len(dst))
            dst[:] = src
        if narrow and poison:  # the bytes of the native plane's region behind the narrow words: not input
            view(slot.input[0] + slot.input_bytes[0], slot.input_bytes[0])[:] = POISON
        for k, a in enumerate(s["states"]):
            view(slot.state[k], slot.state_bytes[k])[:] = np.ascontiguousarray(a).view(np.uint8).ravel()
        live.append((t, int(slot.input_bytes[0]), int(slot.out_bytes), [(int(slot.state[k]), int(slot.state_bytes[k])) for k in range(len(s["states"]))]))
        b.commit(t)
    res = []
    for (t, in0, reserved, state_at), s in zip(live, subs):
        try:
            slot = b.wait(t)
            assert int(slot.input_bytes[0]) == in0
            res.append(dict(status=0, out=view(slot.out, slot.out_bytes).copy(), in0=in0, reserved=reserved,
                            states=[view(slot.state[k], slot.state_bytes[k]).copy() for k in range(len(s["states"]))]))
        except SymaccelError as e:
            res.append(dict(status=e.status, out=None, in0=in0, reserved=reserved, states=[view(p, n).copy() for p, n in state_at]))
        b.release(t)
    st = b.stats()
    b.close()
    return res, st


def native_bytes(s):
    return s["n_chains"] * s["units"] * 4


def assert_twins(subs, modes, wide, got, what):
    """every ticket equals its wide twin: the twin of a ticket with an output format has the same format"""
    for i, (s, (narrow, fmt, ch), r0, r1) in enumerate(zip(subs, modes, wide, got)):
        assert r1["status"] == r0["status"], (what, i, r0["status"], r1["status"])
        assert r1["in0"] == native_bytes(s) // (2 if narrow else 1), (what, i, "input_bytes[0]")
        assert r1["reserved"] == r0["reserved"] == (native_bytes(s) // 4 * BYTES[fmt] if fmt else native_bytes(s)), (what, i, "out_bytes at reserve()")
        for a, bb in zip(r0["states"], r1["states"]):
            assert np.array_equal(a, bb), (what, i, "state planes")
        if r0["status"] == 0:
            assert len(r1["out"]) == len(r0["out"]), (what, i)
            bad = np.flatnonzero(r1["out"] != r0["out"])
            assert bad.size == 0, "%s ticket %d: %d bytes differ from the wide twin, first at %d" % (what, i, bad.size, bad[0])


def versus_wide(ctx, subs, modes, what, poison=False):
    wide, st0 = run_group(ctx, subs, [(False, fmt, ch) for _, fmt, ch in modes])
    got, st1 = run_group(ctx, subs, modes, poison=poison)
    assert_twins(subs, modes, wide, got, what)
    assert (st1["launches"], st1["chunks"], st1["submissions"], st1["failed_tickets"]) == (st0["launches"], st0["chunks"], st0["submissions"], st0["failed_tickets"]), (st0, st1)
    return wide, got, st0, st1


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

def check_shape(ctx, codec, units):
    """three narrow tickets of 3 / 6 / 4 chains (two of 2 chains at 65535 words a row, orders <= 2) in one group"""
    big = units == 65535
    chains = [2, 2] if big else [3, 6, 4]
    subs = [MAKE[codec](1000 * units + i, n, units, max_order=2 if big else 32) for i, n in enumerate(chains)]
    wide, got, st0, _ = versus_wide(ctx, subs, [(True, None, 0)] * len(subs), (codec, units))
    assert st0["launches"] == 1 and st0["failed_tickets"] == 0, st0
    if units == 100:  # ... and the oracle's restore / predict
        for s, r in zip(subs, got):
            assert np.array_equal(r["out"].view(np.int32).reshape(s["n_chains"], units), s["oracle"]()), (codec, "oracle")


MIXED = [(False, None, 0), (True, None, 0), (True, "s16", 2), (False, "s16", 2), (True, "s24", 2)]


def check_mixed(ctx, codec, units, n=5):
    """ONE group of five tickets: wide in / native out, narrow / native, narrow / S16 interleaved, wide / S16, narrow / S24"""
    subs = [MAKE[codec](7000 + units + i, 4 + 2 * (i % 2), units) for i in range(n)]
    modes = [MIXED[i % 5] for i in range(n)]
    wide, got, st0, st1 = versus_wide(ctx, subs, modes, (codec, "mixed", units))
    allwide, st2 = run_group(ctx, subs, [(False, None, 0)] * n)
    assert (st1["launches"], st1["chunks"]) == (st2["launches"], st2["chunks"]), (st1, st2)
    for i in (0, 1):  # native out: the all-wide, all-native run too
        assert np.array_equal(got[i]["out"], allwide[i]["out"])
    return st1


def check_chunking(ctx, codec):
    """(the caller has set SYMACCEL_BATCH_CHUNKS / _CHUNK_MIN_KB): ten tickets of 64 to 96 KiB of native input, a group of many chunks"""
    st = check_mixed(ctx, codec, 4096, n=10)
    assert st["launches"] == 1 and st["chunks"] >= 5, st


def check_param_forms(ctx):
    lib = ctx.lib
    cases = [("flac 0x100 | 16", sub_flac(501, 6, 300, 0x100 | 16)),
             ("flac 0x200 verify", sub_flac_verify(lib, 502, 3, 300, 0x200 | (1 << 12))),
             ("flac 0x300 verify + finish", sub_flac_verify(lib, 503, 3, 300, 0x300 | 16 | (1 << 12))),
             ("alac 0x100", sub_alac(504, 6, 300, 0x100))]
    for what, s in cases:
        wide, got, st0, _ = versus_wide(ctx, [s], [(True, None, 0)], what)
        assert st0["failed_tickets"] == 0 and got[0]["status"] == 0, (what, st0)
        if s["states"]:  # (the checkpoints moved: the case can tell a hashed plane from one that was not)
            assert not np.array_equal(got[0]["states"][0][:len(got[0]["states"][0]) // 3], got[0]["states"][0][-(len(got[0]["states"][0]) // 3):]), what


def check_failing_ticket(ctx):
    """a narrow ticket with a FLAC order above the block size fails alone, with its wide twin's status; its neighbours -- narrow and wide
    -- are bit-equal to a launch without it"""
    subs = [sub_flac(600 + i, 4, 8) for i in range(4)]
    bad = subs[1]
    d = bad["ins"][1].copy()
    d["kind"][1], d["order"][1] = FLAC_LPC, 9
    bad["ins"][1] = d
    modes = [(True, None, 0), (True, None, 0), (False, None, 0), (True, "s16", 2)]
    wide, got, st0, st1 = versus_wide(ctx, subs, modes, "failing ticket")
    assert [r["status"] for r in got] == [0, -1, 0, 0] == [r["status"] for r in wide] and st1["failed_tickets"] == 1, (st0, st1)
    rest = [0, 2, 3]
    without, st = run_group(ctx, [subs[i] for i in rest], [modes[i] for i in rest])
    assert st["failed_tickets"] == 0
    for r, i in zip(without, rest):
        assert r["status"] == 0 and np.array_equal(r["out"], got[i]["out"]), i


def check_refusals(ctx):
    b = Batcher(ctx, 0)
    t, _ = b.reserve(BATCH_FLAC_RESTORE, 0, 2, 16, in_fmt="s16")  # (something live: the counters below are not trivially zero)
    before = b.stats()
    for kind, param, in_fmt in ((BATCH_AAC_SYNTH, 0, "s16"), (BATCH_FLAC_RESTORE, 0, "s8"), (BATCH_ALAC_PREDICT, 0, "s32"), (BATCH_FLAC_RESTORE, 0, 99)):
        with pytest.raises(SymaccelError) as e:
            b.reserve(kind, param, 2, 16, in_fmt=in_fmt)
        assert e.value.status == -1
        buf = np.zeros((2, 16), np.int16)
        with pytest.raises(SymaccelError) as e:
            b.submit(kind, param, [buf, np.zeros(64, np.uint8), np.zeros((2, 32), np.int32)], [np.zeros(4096, np.uint8)], np.zeros((2, 16), np.int32),
                     n_chains=2, units=16, in_fmt=in_fmt)
        assert e.value.status == -1
    after = b.stats()
    assert (after["slots_peak"], after["pending"], after["submissions"]) == (before["slots_peak"], before["pending"], before["submissions"]), (before, after)
    b.release(t)
    assert b.stats()["pending"] == 0
    b.close()


def check_guards(ctx, codec):
    """submit_io, the copy form: the narrow plane comes from caller memory and the bytes around the caller's planes are intact; zero-copy
    form: the slot's bytes behind input_bytes[0] are not read as input"""
    units = 1027
    subs = [MAKE[codec](800 + i, 4, units) for i in range(3)]
    modes = [(True, None, 0), (False, None, 0), (True, "s16", 2)]
    wide, _ = run_group(ctx, subs, [(False, fmt, ch) for _, fmt, ch in modes])
    poisoned, _ = run_group(ctx, subs, modes, poison=True)
    assert_twins(subs, modes, wide, poisoned, (codec, "poison"))
    b = Batcher(ctx, 0)
    held, tickets = [], []
    for s, (narrow, fmt, ch) in zip(subs, modes):
        g = 64
        ins = []
        for k, a in enumerate(s["ins"]):
            a = np.ascontiguousarray(a.astype(np.int16) if k == 0 and narrow else a)
            raw = np.full(a.nbytes + 2 * g, GUARD, np.uint8)
            raw[g:g + a.nbytes] = a.view(np.uint8).ravel()
            ins.append(raw)
        out = np.full(native_bytes(s) + 2 * g, GUARD, np.uint8)
        tickets.append(b.submit(s["kind"], s["param"], [r[g:len(r) - g] for r in ins], [], out[g:len(out) - g], out_format=fmt or 0, channels=ch,
                                n_chains=s["n_chains"], units=units, in_fmt="s16" if narrow else 0))
        held.append((ins, out, g))
    for t in reversed(tickets):
        b.collect(t)
    assert b.stats()["launches"] == 1
    b.close()
    for i, ((ins, out, g), s, r0) in enumerate(zip(held, subs, wide)):
        n = len(r0["out"])
        assert np.array_equal(out[g:g + n], r0["out"]), (codec, i)
        assert np.all(out[:g] == GUARD) and np.all(out[g + n:] == GUARD), (codec, i, "collect() wrote outside out_bytes")
        for k, raw in enumerate(ins):
            a = np.ascontiguousarray(s["ins"][k].astype(np.int16) if k == 0 and modes[i][0] else s["ins"][k]).view(np.uint8).ravel()
            assert np.all(raw[:g] == GUARD) and np.all(raw[len(raw) - g:] == GUARD) and np.array_equal(raw[g:len(raw) - g], a), (codec, i, k)


def small_chunks(monkeypatch):
    monkeypatch.setenv("SYMACCEL_BATCH_CHUNK_MIN_KB", "64")
    monkeypatch.setenv("SYMACCEL_BATCH_CHUNKS", "64")


# ---- symaccel_host_narrow_s16: plain host code ------------------------------------------------------------------------------------------

def narrow(dll, src):
    src = np.ascontiguousarray(src, np.int32)
    dst = np.full(len(src) + 2, 0x7b7b, np.int16)
    r = dll.symaccel_host_narrow_s16(src.ctypes.data, dst[1:].ctypes.data, len(src))
    assert dst[0] == 0x7b7b and dst[-1] == 0x7b7b, "wrote outside dst"
    return r, dst[1:-1]


@pytest.mark.parametrize("n", [1, 7, 8, 33, 1000, 4097])
def test_host_narrow_s16(n):
    dll = emu_library().dll
    rng = np.random.default_rng(n)
    src = rng.integers(-32768, 32768, n).astype(np.int32)
    src[0], src[-1], src[n // 2] = -32768, 32767, -1
    r, dst = narrow(dll, src)
    assert r == 1 and np.array_equal(dst, src)
    for where in sorted({0, n // 2, n - 1}):
        for v in (32768, -32769, (1 << 31) - 1, -(1 << 31), 65536, -65536):
            bad = src.copy()
            bad[where] = v
            assert narrow(dll, bad)[0] == 0, (n, where, v)


def test_host_narrow_s16_of_nothing():
    dll = emu_library().dll
    assert dll.symaccel_host_narrow_s16(None, None, 0) == 1
    assert narrow(dll, np.zeros(0, np.int32))[0] == 1


# ---- CPU emulation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("units", UNITS)
@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_emu_narrow_equals_wide(emu_ctx, codec, units):  # noqa: F811
    check_shape(emu_ctx, codec, units)


@pytest.mark.parametrize("units", [100, 1024])
@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_emu_mixed_group(emu_ctx, codec, units):  # noqa: F811
    check_mixed(emu_ctx, codec, units)


@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_emu_group_cut_into_chunks(emu_ctx, monkeypatch, codec):  # noqa: F811
    small_chunks(monkeypatch)
    check_chunking(emu_ctx, codec)


def test_emu_every_param_form(emu_ctx):  # noqa: F811
    check_param_forms(emu_ctx)


def test_emu_failing_ticket_fails_alone(emu_ctx):  # noqa: F811
    check_failing_ticket(emu_ctx)


def test_emu_refused_requests(emu_ctx):  # noqa: F811
    check_refusals(emu_ctx)


@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_emu_guard_bytes(emu_ctx, codec):  # noqa: F811
    check_guards(emu_ctx, codec)


# ---- the MI355X ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on an MI355X (there is no CPU path)")
    ctx = Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("units", UNITS)
@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_gpu_narrow_equals_wide(gpu_ctx, codec, units):
    check_shape(gpu_ctx, codec, units)


@pytest.mark.gpu
@pytest.mark.parametrize("units", [100, 1024])
@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_gpu_mixed_group(gpu_ctx, codec, units):
    check_mixed(gpu_ctx, codec, units)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_gpu_group_cut_into_chunks(gpu_ctx, monkeypatch, codec):
    small_chunks(monkeypatch)
    check_chunking(gpu_ctx, codec)


@pytest.mark.gpu
def test_gpu_every_param_form(gpu_ctx):
    check_param_forms(gpu_ctx)


@pytest.mark.gpu
def test_gpu_failing_ticket_fails_alone(gpu_ctx):
    check_failing_ticket(gpu_ctx)


@pytest.mark.gpu
def test_gpu_refused_requests(gpu_ctx):
    check_refusals(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_gpu_guard_bytes(gpu_ctx, codec):
    check_guards(gpu_ctx, codec)
