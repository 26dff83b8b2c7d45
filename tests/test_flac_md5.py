"""FLAC stream verification: the STREAMINFO MD5 (symphonia-bundle-flac/src/validate.rs:25-75, decoder.rs:231-234, 272-308) computed
by symaccel_flac_md5(_device), one lane per stream, and the host functions symaccel_md5_*.

What the reference hashes: every decoded frame, decorrelated (decoder.rs:32-82) but BEFORE the `<< (32 - bps)` of decoder.rs:239-242,
each sample truncated to ceil(bps / 8) little-endian bytes, interleaved by channel (copy_as_i8 / i16 / i24 / i32), through
symphonia-core's Md5 -- plain MD5, so `hashlib.md5` of that byte string is the expected digest.  CPU emulation here, gpu-marked twins
on the MI355X."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from emu_lib import emu_ctx, emu_library  # noqa: F401
from symphonia_amd import (FLAC_MD5_JOB_DTYPE, MD5_STATE_DTYPE, flac_bytes_per_sample, flac_md5, flac_md5_device, flac_md5_frames, md5_digest,
                           md5_init, md5_update)

GOLDEN = Path(__file__).resolve().parent / "golden" / "md5_vectors.json"


def _wrap(v):
    return ((np.asarray(v, np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int64)


def decorrelate(mode, a, b):
    """decoder.rs:32-82 on i32 with wrapping arithmetic (as numpy int64)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if mode == 1:
        b = _wrap(a - b)
    elif mode == 2:
        mid = _wrap((a << 1) | (b & 1))
        a, b = _wrap(mid + b) >> 1, _wrap(mid - b) >> 1
    elif mode == 3:
        a = _wrap(a + b)
    return a, b


def pack(rows, nch, block_len, pair_mode, nb):
    """validate.rs: the bytes one stream's frames feed to the MD5."""
    out = []
    for f, n in enumerate(block_len):
        ch = [np.asarray(rows[f * nch + c, :n], np.int64) for c in range(nch)]
        if nch == 2 and pair_mode[f]:
            ch[0], ch[1] = decorrelate(int(pair_mode[f]), ch[0], ch[1])
        inter = np.stack(ch, axis=1).astype(np.int64) & 0xffffffff
        out.append(inter.astype("<u4").view(np.uint8).reshape(n, nch, 4)[:, :, :nb].tobytes())
    return b"".join(out)


def stream_case(seed, nch, bps, n_frames, max_block, pitch=None, modes=True):
    """Random restored subframes (some samples past bps bits, as a damaged frame could give), variable block lengths."""
    rng = np.random.default_rng(seed)
    block_len = rng.integers(1, max_block + 1, n_frames)
    block_len[rng.random(n_frames) < 0.5] = max_block
    pitch = max_block if pitch is None else pitch
    lim = 1 << max(bps - 1, 0)
    rows = rng.integers(-lim, lim, (n_frames * nch, pitch), dtype=np.int64)
    wild = rng.random(rows.shape) < 0.02
    rows[wild] = rng.integers(-(1 << 31), 1 << 31, int(wild.sum()))
    pair_mode = rng.integers(0, 4, n_frames) if (nch == 2 and modes) else np.zeros(n_frames, np.int64)
    return rows.astype(np.int32), block_len, pair_mode


def state_of(data, lib):
    st = md5_init(lib)
    md5_update(st, data, lib)
    return st


def assert_state(got, data, lib):
    """A symaccel_md5_state equals hashlib's after `data`: same digest, same length, and the canonical tail."""
    want = state_of(data, lib)
    assert int(got["len"][0]) == len(data)
    assert md5_digest(got, lib) == hashlib.md5(data).digest()
    assert np.array_equal(got["abcd"], want["abcd"]) and np.array_equal(got["tail"], want["tail"])


# ---- host functions ----------------------------------------------------------------------------------------------------------

def test_host_md5_known_answers():
    lib = emu_library()
    for v in json.loads(GOLDEN.read_text())["vectors"]:
        msg = v["message"].encode("latin-1")
        assert md5_digest(state_of(msg, lib), lib).hex() == v["md5"]
        st = md5_init(lib)  # in pieces of 21 bytes, and byte by byte
        for k in range(0, len(msg), 21):
            md5_update(st, msg[k:k + 21], lib)
        assert md5_digest(st, lib).hex() == v["md5"]
        st = md5_init(lib)
        for k in range(len(msg)):
            md5_update(st, msg[k:k + 1], lib)
        assert md5_digest(st, lib).hex() == v["md5"]
        assert md5_digest(st, lib).hex() == v["md5"]  # the digest does not consume the state


def test_host_md5_lengths_around_the_padding_boundary():
    lib = emu_library()
    rng = np.random.default_rng(1)
    for n in list(range(50, 70)) + [119, 120, 121, 128, 1000]:
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert md5_digest(state_of(msg, lib), lib) == hashlib.md5(msg).digest(), n


# ---- the FLAC path -----------------------------------------------------------------------------------------------------------

def test_known_answers_through_the_flac_path(emu_ctx):
    """The vectors hashed as 8-bit mono frames (sample = the byte as i8), in frames of 1..64 samples: the tail spans frames."""
    lib = emu_ctx.lib
    msgs = [v["message"].encode("latin-1") for v in json.loads(GOLDEN.read_text())["vectors"]]
    msgs += [bytes(range(55)), bytes(range(56)), bytes(range(200))]
    for i, msg in enumerate(msgs):
        for fl in (1, 7, 21, 55, 64, 65):
            blocks = [msg[k:k + fl] for k in range(0, len(msg), fl)] or [b""]
            rows = np.zeros((len(blocks), fl), np.int32)
            for f, blk in enumerate(blocks):
                rows[f, :len(blk)] = np.frombuffer(blk, np.int8)
            frames = flac_md5_frames([len(b) for b in blocks])
            st, cps = flac_md5(emu_ctx, rows, frames, 1, 1, checkpoints=True)
            assert md5_digest(st, lib) == hashlib.md5(msg).digest(), (i, fl)
            done = 0
            for f, blk in enumerate(blocks):
                done += len(blk)
                assert_state(cps[f:f + 1], msg[:done], lib)


@pytest.mark.parametrize("bps", [4, 8, 12, 16, 20, 24, 32])
@pytest.mark.parametrize("nch", [1, 2, 3, 6, 8])
def test_random_streams_match_hashlib(emu_ctx, bps, nch):
    nb = flac_bytes_per_sample(bps)
    rows, bl, pm = stream_case(bps * 10 + nch, nch, bps, 6, 37)
    data = pack(rows, nch, bl, pm, nb)
    st, cps = flac_md5(emu_ctx, rows, flac_md5_frames(bl, pm), nch, nb, checkpoints=True)
    assert_state(st, data, emu_ctx.lib)
    done = 0
    for f in range(len(bl)):
        done += int(bl[f]) * nch * nb
        assert_state(cps[f:f + 1], data[:done], emu_ctx.lib)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_every_pair_mode_with_samples_past_bps(emu_ctx, mode):
    """Samples whose decorrelated values exceed bps bits: the digest is of the truncated pre-shift values, as the reference's."""
    rng = np.random.default_rng(mode)
    n = 4096
    rows = rng.integers(-(1 << 31), 1 << 31, (4, n), dtype=np.int64).astype(np.int32)
    bl, pm = np.array([n, n - 3]), np.array([mode, mode])
    for bps in (16, 24):
        nb = flac_bytes_per_sample(bps)
        st = flac_md5(emu_ctx, rows, flac_md5_frames(bl, pm), 2, nb)
        assert_state(st, pack(rows, 2, bl, pm, nb), emu_ctx.lib)


def test_starting_state_and_unaligned_pitch(emu_ctx):
    """A stream hashed in two calls, the second from the first's state (a tail of 1..63 bytes), rows at an odd pitch."""
    rows, bl, pm = stream_case(5, 2, 24, 5, 33, pitch=35)
    data = pack(rows, 2, bl, pm, 3)
    st = flac_md5(emu_ctx, rows[:4], flac_md5_frames(bl[:2], pm[:2]), 2, 3)
    st = flac_md5(emu_ctx, rows[4:], flac_md5_frames(bl[2:], pm[2:]), 2, 3, state=st)
    assert_state(st, data, emu_ctx.lib)


def test_zero_bytes_per_sample_hashes_nothing(emu_ctx):
    rows, bl, pm = stream_case(6, 2, 16, 3, 16)
    start = state_of(b"xyz", emu_ctx.lib)
    st, cps = flac_md5(emu_ctx, rows, flac_md5_frames(bl, pm), 2, 0, state=start, checkpoints=True)
    assert_state(st, b"xyz", emu_ctx.lib)
    for f in range(3):
        assert_state(cps[f:f + 1], b"xyz", emu_ctx.lib)


def test_host_form_refuses_what_does_not_add_up(emu_ctx):
    from symphonia_amd import SymaccelError
    rows, bl, pm = stream_case(7, 2, 16, 3, 16)
    for args in ((flac_md5_frames([17, 1, 1]), 2, 2), (flac_md5_frames(bl, [0, 4, 0]), 2, 2), (flac_md5_frames(bl, [0, 1, 0]), 1, 2),
                 (flac_md5_frames(bl), 9, 2), (flac_md5_frames(bl), 2, 5)):
        with pytest.raises(SymaccelError):
            flac_md5(emu_ctx, rows, *args)


def md5_jobs_case(seed, n_streams):
    """Several streams of different shapes and lengths, rows at their own pitch, one with a job that does not add up."""
    rng = np.random.default_rng(seed)
    streams = []
    for s in range(n_streams):
        nch = int(rng.choice([1, 2, 2, 3, 6, 8]))
        bps = int(rng.choice([8, 12, 16, 20, 24, 32]))
        max_block = int(rng.integers(1, 300))
        pitch = max_block + int(rng.integers(0, 9))
        rows, bl, pm = stream_case(seed * 1000 + s, nch, bps, int(rng.integers(1, 7)), max_block, pitch=pitch)
        streams.append((rows, bl, pm, nch, flac_bytes_per_sample(bps)))
    return streams


def run_jobs(streams, alloc, lib, hostile=()):
    """Lay the jobs out with `alloc` (numpy array -> (address, keep-alive)) and return the job table and its state / checkpoint planes."""
    keep, jobs = [], np.zeros(len(streams), FLAC_MD5_JOB_DTYPE)
    states = np.zeros(len(streams), MD5_STATE_DTYPE)
    starts = []
    for s, (rows, bl, pm, nch, nb) in enumerate(streams):
        pre = bytes([s]) * (s * 7 % 64)  # every stream starts from a state of its own
        starts.append(pre)
        st = md5_init(lib)
        md5_update(st, pre, lib)
        states[s] = st[0]
        fr = flac_md5_frames(bl, pm)
        if s in hostile:
            fr["pair_mode"][-1] = 5
        jobs[s]["row_pitch"], jobs[s]["n_frames"], jobs[s]["nch"], jobs[s]["bytes_per_sample"] = rows.shape[1], len(bl), nch, nb
        for name, arr in (("rows", rows), ("frames", fr)):
            addr, k = alloc(arr)
            jobs[s][name] = addr
            keep.append(k)
    return jobs, states, starts, keep


def check_jobs(streams, states, cps_list, starts, lib, hostile=()):
    for s, (rows, bl, pm, nch, nb) in enumerate(streams):
        data = pack(rows, nch, bl, pm, nb)
        if s in hostile:
            data = b""
        assert_state(states[s:s + 1], starts[s] + data, lib)
        done = 0
        for f in range(len(bl)):
            done += 0 if s in hostile else int(bl[f]) * nch * nb
            assert_state(cps_list[s][f:f + 1], starts[s] + data[:done], lib)


def test_many_streams_in_one_call(emu_ctx):
    """70 streams (two wavefronts) of different channel counts, widths and lengths in one symaccel_flac_md5_device call; a job that
    does not add up hashes nothing and leaves its neighbours alone."""
    streams = md5_jobs_case(3, 70)
    hostile = (5,)

    def alloc(a):
        a = np.ascontiguousarray(a)
        return a.ctypes.data, a
    jobs, states, starts, keep = run_jobs(streams, alloc, emu_ctx.lib, hostile)
    cps_list = [np.zeros(len(st[1]), MD5_STATE_DTYPE) for st in streams]
    for s in range(len(streams)):
        jobs[s]["state"] = states[s:s + 1].ctypes.data
        jobs[s]["checkpoints"] = cps_list[s].ctypes.data
    flac_md5_device(emu_ctx, jobs)
    check_jobs(streams, states, cps_list, starts, emu_ctx.lib, hostile)


# ---- on the MI355X -----------------------------------------------------------------------------------------------------------

def _gpu_ctx():
    import torch
    from symphonia_amd import Context
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on an MI355X (there is no CPU path)")
    return Context(0)


@pytest.mark.gpu
@pytest.mark.parametrize("bps", [4, 8, 12, 16, 20, 24, 32])
@pytest.mark.parametrize("nch", [1, 2, 3, 6, 8])
def test_gpu_random_streams_match_hashlib(bps, nch):
    nb = flac_bytes_per_sample(bps)
    rows, bl, pm = stream_case(bps * 10 + nch, nch, bps, 6, 300)
    data = pack(rows, nch, bl, pm, nb)
    with _gpu_ctx() as ctx:
        st, cps = flac_md5(ctx, rows, flac_md5_frames(bl, pm), nch, nb, checkpoints=True)
        assert_state(st, data, ctx.lib)
        done = 0
        for f in range(len(bl)):
            done += int(bl[f]) * nch * nb
            assert_state(cps[f:f + 1], data[:done], ctx.lib)


@pytest.mark.gpu
def test_gpu_known_answers_through_the_flac_path():
    msgs = [v["message"].encode("latin-1") for v in json.loads(GOLDEN.read_text())["vectors"]]
    with _gpu_ctx() as ctx:
        for i, msg in enumerate(msgs):
            for fl in (1, 21, 64):
                blocks = [msg[k:k + fl] for k in range(0, len(msg), fl)] or [b""]
                rows = np.zeros((len(blocks), fl), np.int32)
                for f, blk in enumerate(blocks):
                    rows[f, :len(blk)] = np.frombuffer(blk, np.int8)
                st = flac_md5(ctx, rows, flac_md5_frames([len(b) for b in blocks]), 1, 1)
                assert md5_digest(st, ctx.lib) == hashlib.md5(msg).digest(), (i, fl)


@pytest.mark.gpu
def test_gpu_many_streams_in_one_call():
    """The device form over 200 streams (four wavefronts, aligned and unaligned rows) with device planes, one hostile job."""
    import torch
    streams = md5_jobs_case(4, 200)
    hostile = (17, 130)
    with _gpu_ctx() as ctx:
        ctx.use_torch_stream()

        def alloc(a):
            t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).ravel().copy()).cuda()
            return t.data_ptr(), t
        jobs, states, starts, keep = run_jobs(streams, alloc, ctx.lib, hostile)
        d_states = torch.from_numpy(states.view(np.uint8).copy()).cuda()
        d_cps = [torch.zeros(len(st[1]) * MD5_STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for st in streams]
        for s in range(len(streams)):
            jobs[s]["state"] = d_states.data_ptr() + s * MD5_STATE_DTYPE.itemsize
            jobs[s]["checkpoints"] = d_cps[s].data_ptr()
        d_jobs = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
        flac_md5_device(ctx, d_jobs, len(streams))
        torch.cuda.synchronize()
        got_states = d_states.cpu().numpy().view(MD5_STATE_DTYPE)
        got_cps = [c.cpu().numpy().view(MD5_STATE_DTYPE) for c in d_cps]
        check_jobs(streams, got_states, got_cps, starts, ctx.lib, hostile)


def test_frames_with_a_width_of_their_own(emu_ctx):
    """decoder.rs:148-151: a frame header may carry its own bits per sample; the validator hashes each frame at its width."""
    rows, bl, pm = stream_case(8, 2, 24, 6, 40)
    widths = np.array([0, 2, 3, 0, 1, 4])  # 0: the stream's (3)
    data = b"".join(pack(rows[2 * f:2 * f + 2], 2, bl[f:f + 1], pm[f:f + 1], int(widths[f]) or 3) for f in range(6))
    st, cps = flac_md5(emu_ctx, rows, flac_md5_frames(bl, pm, widths), 2, 3, checkpoints=True)
    assert_state(st, data, emu_ctx.lib)


def test_host_form_checks_the_rows_it_is_given(emu_ctx):
    rows, bl, pm = stream_case(9, 2, 16, 3, 16)
    with pytest.raises(ValueError):
        flac_md5(emu_ctx, rows[:5], flac_md5_frames(bl, pm), 2, 2)


def test_a_job_without_a_state_is_skipped(emu_ctx):
    """A job whose state pointer is NULL reads and writes nothing; its neighbours are hashed."""
    streams = md5_jobs_case(11, 3)

    def alloc(a):
        a = np.ascontiguousarray(a)
        return a.ctypes.data, a
    jobs, states, starts, keep = run_jobs(streams, alloc, emu_ctx.lib)
    cps_list = [np.zeros(len(st[1]), MD5_STATE_DTYPE) for st in streams]
    for s in range(len(streams)):
        jobs[s]["state"] = states[s:s + 1].ctypes.data
        jobs[s]["checkpoints"] = cps_list[s].ctypes.data
    jobs[1]["state"] = 0
    flac_md5_device(emu_ctx, jobs)
    assert not cps_list[1].view(np.uint8).any()
    for s in (0, 2):
        rows, bl, pm, nch, nb = streams[s]
        assert_state(states[s:s + 1], starts[s] + pack(rows, nch, bl, pm, nb), emu_ctx.lib)
