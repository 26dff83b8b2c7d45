"""codecs::LookaheadDecoder::set_output / last_decoded_bytes and Context::pcm_convert (include/symaccel.hpp): tests/cpp/pcm_output_test.cpp
decodes synthetic AAC, MP3, Vorbis and two-channel FLAC tracks through a decoder that delivers S16 bytes (converted in the batcher's
scatter) and through one that returns the planar buffer, and compares packet by packet -- across look-ahead batch boundaries and after
reset() -- with the reference's FromSample arithmetic on the host.  CPU: linked against the emulation build of the kernels; GPU: against
libsymaccel.so."""
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "build"
sys.path.insert(0, str(ROOT / "tests" / "emu"))


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
    exe = BUILD / ("pcm_output_test_" + ("emu" if against_emu else "gpu"))
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "pcm_output_test.cpp"), "-o", str(exe),
           "-L", str(so.parent), "-l" + libname, "-Wl,-rpath," + str(so.parent), "-lm", "-pthread"]
    subprocess.run(cmd, check=True)
    return exe


def test_decoders_deliver_s16_bytes_on_the_emulation_build():
    exe = build(against_emu=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_decoders_deliver_s16_bytes_on_the_gpu():
    exe = build(against_emu=False)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
