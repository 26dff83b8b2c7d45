"""A width per row in one batcher submission (in_fmt = SYMACCEL_IN_FMT_ROWS of symaccel_batcher_reserve_io / _submit_io): every row of plane
0 of a FLAC_RESTORE / ALAC_PREDICT ticket at its native offset in the slot, as int16_t, packed little-endian 24-bit or int32_t words, the
widths in slot.input[5]; the gather of the launch widens row by row.

Every comparison is BIT-EQUAL, and the reference is the SAME words sent wide (in_fmt = 0) through a batcher of its own; one shape per kind
is checked against the oracle's restore / predict as well.  A row's words span the whole range of its width; the extreme and the
byte-order-sensitive words of the width stand at the first and the last four words of every row and on both sides of every piece boundary
(4096 words).  The bytes of a row's region behind its valid bytes are poison, two patterns.  The packing here is numpy's, not the
library's.  CPU emulation, and gpu-marked twins of the same cases on the MI355X."""

import numpy as np
import pytest

from emu_lib import emu_ctx, emu_library  # noqa: F401
from symphonia_amd import BATCH_AAC_SYNTH, BATCH_ALAC_PREDICT, BATCH_FLAC_RESTORE, Batcher, Context, SymaccelError
from test_batcher_input_format import MAKE, small_chunks, sub_flac_verify
from test_batcher_output_format import view
from test_pcm_convert import BYTES

UNITS = [1, 3, 17, 100, 1024, 4096, 4097, 4608, 8192, 65535]
PIECE = 4096
POISONS = (0xA5, 0x3C)
GUARD = 0x5A
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
RANGE = {2: (-(1 << 15), 1 << 15), 3: (-(1 << 23), 1 << 23), 4: (I32_MIN, 1 << 31)}
SPECIAL = {2: [-32768, 32767, -1, 0],
           3: [-8388608, 8388607, -1, 0, 0x7F80FE, -0x7F80FE, 0x0180FF, -0x0180FF],  # (three different bytes each: byte order, sign bit)
           4: [I32_MIN, I32_MAX, -1, 0, 0x7F80FE01, -0x7F80FE01]}
PATTERNS = ["all2", "all3", "all4", "cycle", "random"]


def widths_of(pattern, n_chains, rng):
    if pattern == "cycle":
        return np.array([2 + r % 3 for r in range(n_chains)], np.uint8)
    if pattern == "random":
        return rng.integers(2, 5, n_chains).astype(np.uint8)
    return np.full(n_chains, int(pattern[3:]), np.uint8)


def fill_rows(buf, widths, rng):
    """in place (the submission's oracle closure reads the same array): row r holds words of the whole range of widths[r]"""
    n_chains, units = buf.shape
    for r, w in enumerate(widths):
        lo, hi = RANGE[int(w)]
        row = rng.integers(lo, hi, units, dtype=np.int64)
        sp = SPECIAL[int(w)]
        at = list(range(min(4, units))) + list(range(max(0, units - 4), units))
        for edge in range(PIECE, units, PIECE):
            at += [i for i in range(edge - 4, edge + 4) if i < units]
        for k, i in enumerate(at):
            row[i] = sp[(r + k) % len(sp)]
        buf[r] = row.astype(np.int32)


def pack(row, w):
    """the row's words at w bytes each, as bytes"""
    if w == 2:
        assert np.array_equal(row.astype(np.int16), row)
        return row.astype("<i2").view(np.uint8)
    if w == 3:
        assert row.min() >= -(1 << 23) and row.max() < (1 << 23)
        return np.ascontiguousarray(row.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).ravel()
    return row.astype("<i4").view(np.uint8)


def rows_region(buf, widths, poison):
    """the native plane's region of a rows ticket: every row packed at its native offset, poison behind its valid bytes"""
    n_chains, units = buf.shape
    region = np.full(n_chains * units * 4, poison, np.uint8)
    for r, w in enumerate(widths):
        p = pack(buf[r], int(w))
        region[r * units * 4:r * units * 4 + len(p)] = p
    return region


def make(codec, seed, n_chains, units, pattern, param=0, max_order=32, verify_lib=None):
    """a submission whose plane 0 is filled for `pattern` (a width per row; "s16" / "wide": what an S16 / a wide ticket may hold)"""
    rng = np.random.default_rng(seed + 77)
    if verify_lib is not None:
        s = sub_flac_verify(verify_lib, seed, n_chains // 2, units, param)
    else:
        s = MAKE[codec](seed, n_chains, units, param=param, max_order=max_order)
    s["widths"] = widths_of({"s16": "all2", "wide": "all4"}.get(pattern, pattern), n_chains, rng)
    fill_rows(s["ins"][0], s["widths"], rng)
    return s


def run_group(ctx, subs, modes, poison=POISONS[0], tables=None):
    """the submissions through ONE batcher of their own, zero-copy form; modes[i] = (input, out_format, channels), input one of "wide",
    "s16", "rows"; tables[i]: what the width table of ticket i says instead of its own widths.  Per ticket: status, the valid output bytes,
    the state planes; and the batcher's statistics"""
    b = Batcher(ctx, 0)
    live = []
    for i, (s, (inp, fmt, ch)) in enumerate(zip(subs, modes)):
        in_fmt = {"wide": 0, "s16": "s16", "rows": "rows"}[inp]
        t, slot = b.reserve(s["kind"], s["param"], s["n_chains"], s["units"], out_format=fmt or 0, channels=ch, in_fmt=in_fmt)
        native = s["n_chains"] * s["units"] * 4
        assert slot.out == slot.input[0]
        assert int(slot.out_bytes) == (native // 4 * BYTES[fmt] if fmt else native), "out_bytes at reserve()"
        if inp == "rows":
            assert int(slot.input_bytes[0]) == native and int(slot.input_bytes[5]) == s["n_chains"] and slot.input[5]
            view(slot.input[0], native)[:] = rows_region(s["ins"][0], s["widths"], poison)
            view(slot.input[5], s["n_chains"])[:] = (tables or {}).get(i, s["widths"])
        else:
            assert not slot.input[5] and int(slot.input_bytes[5]) == 0
            a = np.ascontiguousarray(s["ins"][0].astype(np.int16) if inp == "s16" else s["ins"][0])
            assert int(slot.input_bytes[0]) == a.nbytes
            view(slot.input[0], a.nbytes)[:] = a.view(np.uint8).ravel()
            if inp == "s16":
                view(slot.input[0] + a.nbytes, a.nbytes)[:] = poison
        for k, a in enumerate(s["ins"][1:], 1):
            a = np.ascontiguousarray(a)
            assert int(slot.input_bytes[k]) == a.nbytes, k
            view(slot.input[k], a.nbytes)[:] = a.view(np.uint8).ravel()
        for k, a in enumerate(s["states"]):
            view(slot.state[k], slot.state_bytes[k])[:] = np.ascontiguousarray(a).view(np.uint8).ravel()
        live.append((t, [(int(slot.state[k]), int(slot.state_bytes[k])) for k in range(len(s["states"]))]))
        b.commit(t)
    res = []
    for (t, state_at), s in zip(live, subs):
        try:
            slot = b.wait(t)
            res.append(dict(status=0, out=view(slot.out, slot.out_bytes).copy(),
                            states=[view(slot.state[k], slot.state_bytes[k]).copy() for k in range(len(s["states"]))]))
        except SymaccelError as e:
            res.append(dict(status=e.status, out=None, states=[view(p, n).copy() for p, n in state_at]))
        b.release(t)
    st = b.stats()
    b.close()
    return res, st


def assert_equal_results(want, got, what):
    for i, (r0, r1) in enumerate(zip(want, got)):
        assert r1["status"] == r0["status"], (what, i, r0["status"], r1["status"])
        for a, bb in zip(r0["states"], r1["states"]):
            assert np.array_equal(a, bb), (what, i, "state planes")
        if r0["status"] == 0:
            assert len(r1["out"]) == len(r0["out"]), (what, i)
            bad = np.flatnonzero(r1["out"] != r0["out"])
            assert bad.size == 0, "%s ticket %d: %d bytes differ from the wide twin, first at %d" % (what, i, bad.size, bad[0])


KEYS = ("launches", "chunks", "submissions", "failed_tickets")


def versus_wide(ctx, subs, modes, what):
    """the group against the same words sent wide (every output format kept), under both poison patterns; launches and chunks as wide"""
    wide, st0 = run_group(ctx, subs, [("wide", fmt, ch) for _, fmt, ch in modes])
    for poison in POISONS:
        got, st1 = run_group(ctx, subs, modes, poison=poison)
        assert_equal_results(wide, got, (what, hex(poison)))
        assert [st1[k] for k in KEYS] == [st0[k] for k in KEYS], (st0, st1)
    return wide, got, st0


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

def check_shape(ctx, codec, units):
    """ONE group of five rows tickets, a width pattern each: all 2, all 3, all 4, the cycle 2 3 4, random"""
    big = units == 65535
    chains = [2] * 5 if big else [4, 6, 4, 6, 8]
    subs = [make(codec, 3000 * units + i, n, units, PATTERNS[i], max_order=2 if big else 32) for i, n in enumerate(chains)]
    wide, got, st0 = versus_wide(ctx, subs, [("rows", None, 0)] * 5, (codec, units))
    assert st0["launches"] == 1 and st0["failed_tickets"] == 0, st0
    if units == 100:  # ... and the oracle's restore / predict
        for s, r in zip(subs, got):
            assert np.array_equal(r["out"].view(np.int32).reshape(s["n_chains"], units), s["oracle"]()), (codec, "oracle")


MIXED = [("wide", None, 0), ("rows", None, 0), ("s16", None, 0), ("rows", "s16", 2), ("s16", "s24", 2), ("rows", "s24", 2), ("wide", "s16", 2),
         ("rows", None, 0), ("rows", "s32", 2), ("rows", None, 0)]
MIXED_PATTERN = ["wide", "cycle", "s16", "random", "s16", "all3", "wide", "all2", "cycle", "all4"]


def check_mixed(ctx, codec, units, n=7, param=0):
    """ONE group of rows, S16 and wide tickets, with and without an output format"""
    subs = [make(codec, 9000 + units + i, 4 + 2 * (i % 2), units, MIXED_PATTERN[i % 10], param=param) for i in range(n)]
    modes = [MIXED[i % 10] for i in range(n)]
    wide, got, st0 = versus_wide(ctx, subs, modes, (codec, "mixed", units, hex(param)))
    assert st0["failed_tickets"] == 0, st0
    allwide, st2 = run_group(ctx, subs, [("wide", None, 0)] * n)
    assert (st0["launches"], st0["chunks"]) == (st2["launches"], st2["chunks"]), (st0, st2)
    for i, m in enumerate(modes):  # native out: the all-wide, all-native run too
        if m[1] is None:
            assert np.array_equal(got[i]["out"], allwide[i]["out"]), i
    return st0


def check_chunking(ctx, codec):
    """(the caller has set SYMACCEL_BATCH_CHUNKS / _CHUNK_MIN_KB): ten tickets of 64 to 96 KiB of native input, a group of many chunks"""
    st = check_mixed(ctx, codec, 4096, n=10)
    assert st["launches"] == 1 and st["chunks"] >= 5, st


def check_param_forms(ctx):
    """the stereo forms, the verify and the finishing form: a rows ticket alone, cycle of widths"""
    lib = ctx.lib
    cases = [("flac 0x100 | 16", make("flac", 511, 6, 300, "cycle", param=0x100 | 16)),
             ("flac 0x200 verify", make("flac", 512, 6, 300, "cycle", param=0x200 | (1 << 12), verify_lib=lib)),
             ("flac 0x300 verify + finish", make("flac", 513, 6, 300, "random", param=0x300 | 16 | (1 << 12), verify_lib=lib)),
             ("alac 0x100", make("alac", 514, 6, 300, "cycle", param=0x100))]
    for what, s in cases:
        wide, got, st0 = versus_wide(ctx, [s], [("rows", None, 0)], what)
        assert st0["failed_tickets"] == 0 and got[0]["status"] == 0, (what, st0)
        if s["states"]:  # (the checkpoints moved: the case can tell a hashed plane from one that was not)
            st = got[0]["states"][0]
            assert not np.array_equal(st[:len(st) // 3], st[-(len(st) // 3):]), what
    # ... and the stereo forms in a mixed group
    check_mixed(ctx, "flac", 300, n=5, param=0x100 | 16)
    check_mixed(ctx, "alac", 300, n=5, param=0x100)


def check_bad_width(ctx, codec, bad):
    """a width byte that is none of 2, 3, 4 in ONE ticket: that ticket fails alone with status -1, its neighbours -- rows, S16, wide --
    are bit-equal to a launch without it"""
    subs = [make(codec, 650 + i, 4, 37, p) for i, p in enumerate(["cycle", "all3", "s16", "wide", "random"])]
    modes = [("rows", None, 0), ("rows", None, 0), ("s16", None, 0), ("wide", "s16", 2), ("rows", "s24", 2)]
    rest = [0, 2, 3, 4]
    without, st = run_group(ctx, [subs[i] for i in rest], [modes[i] for i in rest])
    assert st["failed_tickets"] == 0 and all(r["status"] == 0 for r in without)
    for where in (0, 3):  # (the rows are packed by the ticket's own widths; only the table's byte is bad)
        table = subs[1]["widths"].copy()
        table[where] = bad
        got, st1 = run_group(ctx, subs, modes, tables={1: table})
        assert [r["status"] for r in got] == [0, -1, 0, 0, 0], (bad, where, [r["status"] for r in got])
        assert st1["failed_tickets"] == 1 and st1["launches"] == 1, st1
        for r, i in zip(without, rest):
            assert np.array_equal(r["out"], got[i]["out"]), (bad, where, i)


def check_refusals(ctx):
    b = Batcher(ctx, 0)
    t, _ = b.reserve(BATCH_FLAC_RESTORE, 0, 2, 16, in_fmt="rows")  # (something live: the counters below are not trivially zero)
    before = b.stats()
    for kind, param, in_fmt in ((BATCH_AAC_SYNTH, 0, "rows"), (BATCH_FLAC_RESTORE, 0, "s8"), (BATCH_ALAC_PREDICT, 0, "s32"), (BATCH_FLAC_RESTORE, 0, 99)):
        with pytest.raises(SymaccelError) as e:
            b.reserve(kind, param, 2, 16, in_fmt=in_fmt)
        assert e.value.status == -1
        with pytest.raises(SymaccelError) as e:
            b.submit(kind, param, [np.zeros(2 * 16 * 4, np.uint8), np.zeros(64, np.uint8), np.zeros((2, 32), np.int32), None, None, np.full(2, 2, np.uint8)],
                     [np.zeros(4096, np.uint8)], np.zeros((2, 16), np.int32), n_chains=2, units=16, in_fmt=in_fmt)
        assert e.value.status == -1
    # the copying form without a width table
    with pytest.raises(SymaccelError) as e:
        b.submit(BATCH_FLAC_RESTORE, 0, [np.zeros(2 * 16 * 4, np.uint8), np.zeros(64, np.uint8), np.zeros((2, 32), np.int32)], [], np.zeros((2, 16), np.int32),
                 n_chains=2, units=16, in_fmt="rows")
    assert e.value.status == -1
    after = b.stats()
    assert (after["slots_peak"], after["pending"], after["submissions"]) == (before["slots_peak"], before["pending"], before["submissions"]), (before, after)
    b.release(t)
    assert b.stats()["pending"] == 0
    b.close()


def check_guards(ctx, codec):
    """submit_io / collect, the copying forms: rows and width table come from caller memory; the bytes around the caller's arrays are intact
    and collect() writes out_bytes and no more"""
    units = 1027
    pats = ["cycle", "wide", "random", "all3"]
    subs = [make(codec, 820 + i, 4, units, p) for i, p in enumerate(pats)]
    modes = [("rows", None, 0), ("wide", None, 0), ("rows", "s16", 2), ("rows", "s24", 2)]
    wide, _ = run_group(ctx, subs, [("wide", fmt, ch) for _, fmt, ch in modes])
    b = Batcher(ctx, 0)
    held, tickets = [], []
    g = 64
    for s, (inp, fmt, ch) in zip(subs, modes):
        arrays = [np.ascontiguousarray(a).view(np.uint8).ravel() for a in s["ins"]]
        if inp == "rows":
            arrays[0] = rows_region(s["ins"][0], s["widths"], POISONS[1])
            arrays += [None] * (5 - len(arrays)) + [s["widths"].copy()]
        raws = []
        for a in arrays:
            if a is None:
                raws.append(None)
                continue
            raw = np.full(a.nbytes + 2 * g, GUARD, np.uint8)
            raw[g:g + a.nbytes] = a
            raws.append(raw)
        out = np.full(s["n_chains"] * units * 4 + 2 * g, GUARD, np.uint8)
        tickets.append(b.submit(s["kind"], s["param"], [None if r is None else r[g:len(r) - g] for r in raws], [], out[g:len(out) - g], out_format=fmt or 0,
                                channels=ch, n_chains=s["n_chains"], units=units, in_fmt="rows" if inp == "rows" else 0))
        held.append((arrays, raws, out))
    for t in reversed(tickets):
        b.collect(t)
    assert b.stats()["launches"] == 1 and b.stats()["failed_tickets"] == 0
    b.close()
    for i, ((arrays, raws, out), r0) in enumerate(zip(held, wide)):
        n = len(r0["out"])
        assert np.array_equal(out[g:g + n], r0["out"]), (codec, i)
        assert np.all(out[:g] == GUARD) and np.all(out[g + n:] == GUARD), (codec, i, "collect() wrote outside out_bytes")
        for k, (a, raw) in enumerate(zip(arrays, raws)):
            if raw is not None:
                assert np.all(raw[:g] == GUARD) and np.all(raw[len(raw) - g:] == GUARD) and np.array_equal(raw[g:len(raw) - g], a), (codec, i, k)


# ---- symaccel_host_pack_row: plain host code --------------------------------------------------------------------------------------------

def pack_row(dll, src):
    src = np.ascontiguousarray(src, np.int32)
    dst = np.full(4 * len(src) + 16, 0x7B, np.uint8)
    w = dll.symaccel_host_pack_row(src.ctypes.data, dst[8:].ctypes.data, len(src))
    assert w in (2, 3, 4)
    assert np.all(dst[:8] == 0x7B) and np.all(dst[8 + w * len(src):] == 0x7B), "wrote outside n * width bytes"
    return w, dst[8:8 + w * len(src)]


def unpack(raw, w):
    if w == 2:
        return raw.view("<i2").astype(np.int32)
    if w == 4:
        return raw.view("<i4").astype(np.int32)
    b = raw.reshape(-1, 3).astype(np.int32)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.int32)


@pytest.mark.parametrize("n", [1, 7, 16, 33, 1000, 4097])
def test_host_pack_row(n):
    dll = emu_library().dll
    rng = np.random.default_rng(n)
    base = rng.integers(-100, 100, n).astype(np.int32)
    for where in sorted({0, n // 2, n - 1}):
        for extreme, want in ((0, 2), (32767, 2), (-32768, 2), (32768, 3), (-32769, 3), (8388607, 3), (-8388608, 3), (8388608, 4), (-8388609, 4),
                              (I32_MAX, 4), (I32_MIN, 4)):
            src = base.copy()
            src[where] = extreme
            w, raw = pack_row(dll, src)
            assert w == want, (n, where, extreme, w)
            assert np.array_equal(unpack(raw, w), src), (n, where, extreme)
    for w0 in (2, 3, 4):  # the whole range of a width, and numpy's packing of it
        src = rng.integers(*RANGE[w0], n, dtype=np.int64).astype(np.int32)
        src[0] = RANGE[w0][0]
        w, raw = pack_row(dll, src)
        assert w == w0 and np.array_equal(raw, pack(src, w0)) and np.array_equal(unpack(raw, w), src)


def test_host_pack_row_of_nothing():
    dll = emu_library().dll
    assert dll.symaccel_host_pack_row(None, None, 0) == 2
    assert pack_row(dll, np.zeros(0, np.int32))[0] == 2


def test_python_host_pack_row():
    from symphonia_amd import host_pack_row
    w, raw = host_pack_row(np.array([1, -8388608, 0x7F80FE], np.int32), lib=emu_library())
    assert w == 3 and raw.tolist() == [1, 0, 0, 0, 0, 0x80, 0xFE, 0x80, 0x7F]


# ---- CPU emulation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("units", UNITS)
@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_emu_rows_equal_wide(emu_ctx, codec, units):  # noqa: F811
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


@pytest.mark.parametrize("bad", [0, 1, 5, 255])
@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_emu_bad_width_fails_alone(emu_ctx, codec, bad):  # noqa: F811
    check_bad_width(emu_ctx, codec, bad)


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
def test_gpu_rows_equal_wide(gpu_ctx, codec, units):
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
@pytest.mark.parametrize("bad", [0, 1, 5, 255])
@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_gpu_bad_width_fails_alone(gpu_ctx, codec, bad):
    check_bad_width(gpu_ctx, codec, bad)


@pytest.mark.gpu
def test_gpu_refused_requests(gpu_ctx):
    check_refusals(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_gpu_guard_bytes(gpu_ctx, codec):
    check_guards(gpu_ctx, codec)
