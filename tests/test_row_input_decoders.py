"""codecs::Flac behind LookaheadDecoder sending every row (subframe) at a width of its own (SYMACCEL_NARROW_INPUT=2,
Batcher::InputMode::Rows; the header has no ALAC codec): tests/cpp/row_input_decoders_test.cpp is handed six streams made here -- per
packet the words, descriptors and coefficients the front end would hand over, the PCM the oracle restores from them (decorrelated and
left-justified in numpy) and hashlib's MD5 of the stream.  Three are 16-bit streams (one of them with ONE 17-bit side warm-up in packet
5), three are 24-bit streams whose VERBATIM subframes span the whole 24-bit range (one of them with ONE 25-bit side warm-up).  The program
runs once per mode -- 0 (unset: wide), 1 (whole batches narrow), 2 (a width per row) -- and checks in each that the PCM is the oracle's,
that the rows sent per width are what the words need, and that the bytes of plane 0 are the sum the widths give.
CPU: linked against the emulation build of the kernels; GPU: against libsymaccel.so."""
import hashlib
import os
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle
from test_flac_md5 import decorrelate, pack

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "build"
sys.path.insert(0, str(ROOT / "tests" / "emu"))

N_PACKETS = 13


def flac_stream(seed, nch, bps, max_bs, wide_at=None):
    """packets whose every word fits `bps` bits: VERBATIM subframes over the whole range (its two ends among them), small residuals behind
    small warm-ups for the predictors.  wide_at: that packet is left/side and its side channel starts with a (bps + 1)-bit warm-up"""
    rng = np.random.default_rng(seed)
    nb, shift, top = bps // 8, 32 - bps, 1 << (bps - 1)
    out, hashed = [], []
    for i in range(N_PACKETS):
        bs = max_bs if i % 3 else int(rng.integers(33, max_bs + 1))
        kind = rng.integers(0, 3, nch).astype(np.uint8)
        if i == 0:
            kind[0] = 0  # (at least one VERBATIM subframe: a 24-bit stream has rows that need their 3 bytes)
        order = np.minimum(np.where(kind == 1, rng.integers(0, 5, nch), rng.integers(1, 33, nch)), bs).astype(np.uint8)
        kind[(kind == 2) & (order == 0)] = 0
        words = rng.integers(-top, top, (nch, bs), dtype=np.int64)
        words[:, 0], words[:, -1] = -top, top - 1
        words[kind != 0] = rng.integers(-40, 40, (int((kind != 0).sum()), bs))
        mode = int(rng.integers(0, 4)) if nch == 2 else 0
        if i == wide_at:
            mode, kind[1], order[1] = 1, 1, 2
            words[1] = rng.integers(-40, 40, bs)
            words[1, 0] = top + top // 4
        assert i == wide_at or ((words >= -top) & (words < top)).all()
        words = words.astype(np.int32)
        desc = oracle.flac_desc(kind, order, rng.integers(0, 12, nch), np.where(rng.random(nch) < 0.2, 1, 0))
        coeffs = rng.integers(-(1 << 9), 1 << 9, (nch, 32)).astype(np.int32)
        restored = oracle.flac_restore(words, desc, coeffs)
        hashed.append(pack(restored, nch, [bs], [mode], nb))
        ch = [restored[c].astype(np.int64) for c in range(nch)]
        if mode:
            ch[0], ch[1] = decorrelate(mode, ch[0], ch[1])
        pcm = np.stack([((c & 0xffffffff) << shift & 0xffffffff).astype(np.uint32).view(np.int32) for c in ch])
        out.append(struct.pack("<II", bs, mode) + words.tobytes() + np.ascontiguousarray(desc, np.uint8).tobytes() + coeffs.tobytes() + pcm.tobytes())
    return struct.pack("<IIII", nch, bps, max_bs, N_PACKETS) + hashlib.md5(b"".join(hashed)).digest() + b"".join(out)


def case_file():
    BUILD.mkdir(exist_ok=True)
    path = BUILD / "row_input_decoders_cases.bin"
    path.write_bytes(struct.pack("<I", 6) + flac_stream(1, 2, 16, 192) + flac_stream(1, 2, 16, 192, wide_at=5) + flac_stream(3, 3, 16, 150) +
                     flac_stream(5, 2, 24, 1024) + flac_stream(5, 2, 24, 1024, wide_at=5) + flac_stream(6, 1, 24, 4097))
    return path


def build(against_emu):
    if against_emu:
        import build_emu
        so = build_emu.build()
        libname = "symaccel_emu"
    else:
        from symphonia_amd import build as sa_build
        so = sa_build.build()
        libname = "symaccel"
    BUILD.mkdir(exist_ok=True)
    exe = BUILD / ("row_input_decoders_test_" + ("emu" if against_emu else "gpu"))
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "row_input_decoders_test.cpp"), "-o", str(exe),
           "-L", str(so.parent), "-l" + libname, "-Wl,-rpath," + str(so.parent), "-lm", "-pthread"]
    subprocess.run(cmd, check=True)
    return exe


def run_twin(against_emu):
    exe, cases = build(against_emu), case_file()
    env = {k: v for k, v in os.environ.items() if k != "SYMACCEL_NARROW_INPUT"}
    for mode in ("0", "1", "2"):
        extra = {"SYMACCEL_NARROW_INPUT": mode} if mode != "0" else {}
        r = subprocess.run([str(exe), str(cases), mode], capture_output=True, text=True, timeout=300, env=dict(env, **extra))
        assert r.returncode == 0 and "all checks passed" in r.stdout, "mode " + mode + ": " + r.stdout[-3000:] + r.stderr[-2000:]


def test_cpp_twin_on_the_emulation_build():
    run_twin(against_emu=True)


@pytest.mark.gpu
def test_cpp_twin_on_the_gpu():
    run_twin(against_emu=False)
