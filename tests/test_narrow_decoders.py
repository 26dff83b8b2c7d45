"""The FLAC / ALAC decoders sending their batches up as 16-bit words (symaccel_batcher_reserve_io) when every word of a batch fits.

C++ (codecs::Flac behind LookaheadDecoder; the header has no ALAC codec): tests/cpp/narrow_decoders_test.cpp is handed five streams made
here -- per packet the words, descriptors and coefficients the front end would hand over, the PCM the oracle restores from them
(decorrelated and left-justified in numpy) and hashlib's MD5 of the stream.  Four fit int16_t in every word (two and three channels, 16
bits); the fifth is the first with ONE 17-bit side warm-up put into packet 5.  The program is run with SYMACCEL_NARROW_INPUT=1 ("on": no
batch of the four goes wide, exactly one of the fifth does) and without it ("off": none goes narrow); the PCM is the oracle's both times,
and finalize() is Some(true) when verifying.  CPU: linked against the emulation build of the kernels; GPU: against libsymaccel.so.

Rust shim (HipFlacDecoder / HipAlacDecoder, executed by tools/rsinterp; needs the reference tree: `localref`): written 16-bit stereo
streams from the writers and fixtures of tests/test_flac_packets.py / test_alac_packets.py, decoded behind a look-ahead reader through the
registry with SYMACCEL_NARROW_INPUT=1: every packet's PCM is the reference decoder's, across the look-ahead batch boundaries and after
reset(); every batch that went to the batcher went narrow (wide_batches() == 0: the writers' amplitude -- 0.8 of a quarter of full scale
per channel -- keeps every side sample inside 16 bits, which this very assertion checks); without the variable none does."""
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


def flac_stream(seed, nch, max_bs, wide_at=None):
    """16-bit packets whose every word fits int16_t: VERBATIM subframes over the whole 16-bit range (-32768 and 32767 among them), small
    residuals behind small warm-ups for the predictors.  wide_at: that packet is left/side and its side channel starts with 40000"""
    rng = np.random.default_rng(seed)
    bps, nb, shift = 16, 2, 16
    out, hashed = [], []
    for i in range(N_PACKETS):
        bs = max_bs if i % 3 else int(rng.integers(33, max_bs + 1))
        kind = rng.integers(0, 3, nch).astype(np.uint8)
        order = np.minimum(np.where(kind == 1, rng.integers(0, 5, nch), rng.integers(1, 33, nch)), bs).astype(np.uint8)
        kind[(kind == 2) & (order == 0)] = 0
        words = rng.integers(-(1 << 15), 1 << 15, (nch, bs), dtype=np.int64)
        words[:, 0], words[:, -1] = -32768, 32767
        words[kind != 0] = rng.integers(-40, 40, (int((kind != 0).sum()), bs))
        mode = int(rng.integers(0, 4)) if nch == 2 else 0
        if i == wide_at:
            mode, kind[1], order[1] = 1, 1, 2
            words[1] = rng.integers(-40, 40, bs)
            words[1, 0] = 40000
        assert i == wide_at or (np.abs(words + 0.5) < 32768).all()
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
    path = BUILD / "narrow_decoders_cases.bin"
    path.write_bytes(struct.pack("<I", 5) + flac_stream(1, 2, 192) + flac_stream(2, 2, 1024) + flac_stream(3, 3, 150) + flac_stream(4, 1, 4097) +
                     flac_stream(1, 2, 192, wide_at=5))
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
    exe = BUILD / ("narrow_decoders_test_" + ("emu" if against_emu else "gpu"))
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "narrow_decoders_test.cpp"), "-o", str(exe),
           "-L", str(so.parent), "-l" + libname, "-Wl,-rpath," + str(so.parent), "-lm", "-pthread"]
    subprocess.run(cmd, check=True)
    return exe


def run_twin(against_emu):
    exe, cases = build(against_emu), case_file()
    env = {k: v for k, v in os.environ.items() if k != "SYMACCEL_NARROW_INPUT"}
    for mode, extra in (("on", {"SYMACCEL_NARROW_INPUT": "1"}), ("off", {})):
        r = subprocess.run([str(exe), str(cases), mode], capture_output=True, text=True, timeout=300, env=dict(env, **extra))
        assert r.returncode == 0 and "all checks passed" in r.stdout, mode + ": " + r.stdout[-3000:] + r.stderr[-2000:]


def test_cpp_twin_on_the_emulation_build():
    run_twin(against_emu=True)


@pytest.mark.gpu
def test_cpp_twin_on_the_gpu():
    run_twin(against_emu=False)


# ---- the Rust shim under the interpreter ----------------------------------------------------------------------------------------------

def shim_run(monkeypatch, codec, narrow):
    """one written 16-bit stereo stream behind a look-ahead reader, a decoder from the registry: 8 packets (two look-ahead batches and
    more), a seek back to packet 3 with reset(), 4 packets again.  Returns (narrow batches, wide batches, batcher statistics)"""
    from emu_lib import emu_library
    from rs_harness import Harness, pool_stats, registry_round_trip, usize
    from rsinterp import interp as I
    if narrow:
        monkeypatch.setenv("SYMACCEL_NARROW_INPUT", "1")
    else:
        monkeypatch.delenv("SYMACCEL_NARROW_INPUT", raising=False)
    n, depth = 8, 4
    if codec == "flac":
        import flac_writer as W
        import test_flac_packets as T
        nch, bps, unit = 2, 16, 192
        ref_tree, tree = T.REF / "symphonia-bundle-flac" / "src", T.patched_tree(("symphonia-bundle-flac",)) / "symphonia-bundle-flac" / "src"
        packets, _ = W.random_stream(41, n, nch, bps, unit)
        name, cpu_name, adapter, trees = "HipFlacDecoder", "FlacDecoder", "flac.rs", dict(flac_tree=tree)
        ref = Harness(None, reference=True, flac_tree=ref_tree)
        ref_dec = T.cpu_decoder(ref, nch, bps, unit)
        params = lambda h: h.params("CODEC_ID_FLAC", extra=T.streaminfo(unit, 44100, nch, bps))  # noqa: E731
    else:
        import test_alac_packets as T
        nch, bps, unit = 2, 16, 128
        ref_tree, tree = T.REF / T.CRATE / "src", T.patched_tree((T.CRATE,)) / T.CRATE / "src"
        packets, _ = T.stream(43, n, nch, bps, unit)
        name, cpu_name, adapter, trees = "HipAlacDecoder", "AlacDecoder", "alac.rs", dict(alac_tree=tree)
        ref = Harness(None, reference=True, alac_tree=ref_tree)
        ref_dec = T.cpu_decoder(ref, nch, bps, unit)
        params = lambda h: h.params("CODEC_ID_ALAC", extra=T.W.cookie(unit, bps, nch))  # noqa: E731
    want = []
    for i, d in enumerate(packets):  # the reference decoder's PCM
        st, planes = ref.decode(cpu_name, ref_dec, ref.packet(d, i * unit))
        assert st == "ok", (i, planes)
        want.append(planes)
    h = Harness(emu_library().dll, reference=True, **trees)
    h.it.load_file(ROOT / "tests" / "rust" / "registry_stubs.rs")
    h.it.load_file(ROOT / "tests" / "rust" / "mocks.rs")
    h.load_shim("lib.rs", "ctx.rs", "decoder.rs", "lookahead.rs", "fallback.rs", adapter, "frontends.rs")
    dec = registry_round_trip(h, name, [params(h)])[0]
    pk = I.Arr([h.packet(d, i * unit, track=1, owned=True) for i, d in enumerate(packets)], True)
    reader = h.it.call("LookaheadReader::new", h.it.call("MockReader::new", pk), usize(depth))

    def run(first, count):
        for i in range(first, first + count):
            r = h.it.call_method("LookaheadReader", "next_packet", reader)
            st, got = h.decode(name, dec, h.it.call_method("Packet", "as_packet_ref", r.f["0"].f["0"]))
            assert st == "ok" and np.array_equal(got, want[i]), (codec, narrow, i)

    run(0, n)
    h.it.call_method("LookaheadReader", "seek", reader, I.Int(0, "i64"), usize(3))
    h.it.call_method(name, "reset", dec)
    run(3, 4)
    counts = [int(h.it.call_method(name, m, dec).v) for m in ("narrow_batches", "wide_batches")]
    calls = h.bridge.calls
    assert calls.count("symaccel_batcher_reserve_io") == counts[0] and calls.count("symaccel_batcher_reserve") == counts[1], (counts, calls.count("symaccel_batcher_reserve"))
    return counts[0], counts[1], pool_stats(h)


@pytest.mark.localref
@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_rust_shim_sends_fitting_batches_narrow(monkeypatch, codec):
    nb, wb, stats = shim_run(monkeypatch, codec, narrow=True)
    assert wb == 0 and nb >= 2, (nb, wb)
    assert stats["submissions"] == nb and stats["failed_tickets"] == 0, stats


@pytest.mark.localref
def test_rust_shim_stays_wide_without_the_variable(monkeypatch):
    nb, wb, stats = shim_run(monkeypatch, "flac", narrow=False)
    assert nb == 0 and wb >= 2 and stats["failed_tickets"] == 0, (nb, wb, stats)
