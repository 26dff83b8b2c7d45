"""codecs::CodecBase (include/symaccel.hpp): tests/cpp/codec_base_test.cpp puts a toy codec that supplies the required members and no
hook behind LookaheadDecoder -- every buffer across a batch boundary and after a skipped packet (the replay), and what every default
means seen from outside (finalize(), set_verify() in mid-stream, the narrow / wide counts) -- and pins the constants the codecs
override.  CPU: linked against the emulation build of the kernels; GPU: against libsymaccel.so."""
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
    exe = BUILD / ("codec_base_test_" + ("emu" if against_emu else "gpu"))
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "codec_base_test.cpp"), "-o", str(exe),
           "-L", str(so.parent), "-l" + libname, "-Wl,-rpath," + str(so.parent), "-lm", "-pthread"]
    subprocess.run(cmd, check=True)
    return exe


def test_codec_base_defaults_on_the_emulation_build():
    exe = build(against_emu=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_codec_base_defaults_on_the_gpu():
    exe = build(against_emu=False)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
