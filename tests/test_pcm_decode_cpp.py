"""codecs::Pcm behind LookaheadDecoder, register_pcm and Context::pcm_decode (include/symaccel.hpp) against the reference fixture:
tests/cpp/pcm_decode_test.cpp is handed the packets, planes and try_new refusals of tests/golden/pcm_decode.npz (the reference's own
PcmDecoder under the interpreter) in a flat file and compares, bit for bit, the direct call, a decoder made by CodecRegistry on the shared
batcher across look-ahead batch boundaries and after reset(), a decoder without a batcher and S16 delivery; the constructor's errors carry
the reference's variants.  CPU: linked against the emulation build of the kernels; GPU: against libsymaccel.so."""
import json
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "tests" / "cpp" / "build"
GOLDEN = ROOT / "tests" / "golden" / "pcm_decode.npz"
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT / "tests"))

import pcm_decode_ref as R  # noqa: E402


def export_fixture(path):
    """the fixture's decoder cases and refusals as little-endian u32 fields and raw bytes (the layout tests/cpp/pcm_decode_test.cpp reads)"""
    z = np.load(GOLDEN)
    m = json.loads(bytes(z["manifest"]).decode())
    cases = [e for e in m["entries"] if "packets" in e]
    out = [b"PCMF", struct.pack("<I", len(cases))]
    for e in cases:
        fam = R.CODECS[e["codec"]][3]
        w, nb = R.WIDTH[fam], R.native_bytes(e["codec"])
        bps, bpcs = (w, w - e["shift"]) if e["shift"] else (0, 0)
        out.append(struct.pack("<8I", R.NAMES.index(e["codec"]) + 1, e["channels"], e["shift"], bps, bpcs, e["max_frames_per_packet"], nb, len(e["packets"])))
        for j, pk in enumerate(e["packets"]):
            data, planes = z["%s_p%d_bytes" % (e["name"], j)], np.ascontiguousarray(z["%s_p%d_planes" % (e["name"], j)])
            assert planes.dtype.itemsize == nb and planes.shape == (e["channels"], pk["frames"])
            out += [struct.pack("<2I", len(data), pk["frames"]), data.tobytes(), planes.tobytes()]
    out.append(struct.pack("<I", len(m["try_new_refusals"])))
    for r in m["try_new_refusals"]:
        name = r["codec"].replace("CODEC_ID_PCM_", "").lower()
        out.append(struct.pack("<6I", R.NAMES.index(name) + 1 if name in R.NAMES else 0, r["sample_rate"] or 0, r["channels"] or 0, r["bits_per_sample"] or 0,
                               r["bits_per_coded_sample"] or 0, {"Unsupported": 1, "DecodeError": 2}[r["error"]]))
    path.write_bytes(b"".join(out))
    return len(cases)


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
    exe = BUILD / ("pcm_decode_test_" + ("emu" if against_emu else "gpu"))
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "pcm_decode_test.cpp"), "-o", str(exe),
           "-L", str(so.parent), "-l" + libname, "-Wl,-rpath," + str(so.parent), "-lm", "-pthread"]
    subprocess.run(cmd, check=True)
    return exe


def run(against_emu, tmp_path):
    flat = tmp_path / "pcm_decode_fixture.bin"
    assert export_fixture(flat) == 34  # the fourteen integer codecs at two shifts, the four float and two log codecs at one
    exe = build(against_emu)
    r = subprocess.run([str(exe), str(flat)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_pcm_twin_on_the_emulation_build(tmp_path):
    run(True, tmp_path)


@pytest.mark.gpu
def test_pcm_twin_on_the_gpu(tmp_path):
    run(False, tmp_path)
