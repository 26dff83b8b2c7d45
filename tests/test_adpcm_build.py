"""The ADPCM decode kernels at the ISA level, read from the device assembly of the translation unit the product builds
them in (batch_copy.hip includes adpcm.hip), with the product's flags: 3 codecs x mono / stereo x 5 output widths = 30 kernels, and for each

  * no scratch, and at most 16 KiB of LDS (ten one-wavefront workgroups per compute unit);
  * block bytes arrive in 16-byte loads -- the only others are byte loads (a unit that reaches outside the input: the first and the last
    of a launch) and the two dword loads that copy the tables into LDS;
  * PCM leaves in 16-byte stores -- the only others are the stores of the up to 15 bytes at either end of a run that fill no aligned
    unit (dword, short or byte stores by the sample size, a handful of instructions) and the status byte; nothing 8 or 12 bytes wide;
  * no fused f32 arithmetic (the F32 output is one exact multiplication by 2^-15).
"""
import re
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tools.kernel_resources import device_asm, kernel_resources  # noqa: E402

LOADS = re.compile(r"\b(?:global|flat)_load_(\w+)")
STORES = re.compile(r"\b(?:global|flat)_store_(\w+)")
F32_FUSED = re.compile(r"\b(v_fma_f32|v_fmac_f32|v_mac_f32|v_mad_f32|v_pk_fma_f32|v_fma_mix\w*|v_mad_mix\w*)\b")


@pytest.fixture(scope="module")
def listing():
    if not (shutil.which("hipcc") or Path("/opt/rocm/bin/hipcc").exists()):
        pytest.skip("hipcc not available")
    return device_asm("batch_copy.hip")


def bodies(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M) if "adpcm_decode_kernel" in m.group(1)}


def test_thirty_kernels_without_scratch(listing):
    res = {n: r for n, r in kernel_resources(listing).items() if "adpcm_decode_kernel" in n}
    assert len(res) == 30, sorted(res)
    for name, r in res.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["LDSByteSize"] <= 16 * 1024 and r["NumVgprs"] <= 168, (name, r)


def test_global_accesses_are_sixteen_bytes_wide_except_at_edges(listing):
    kernels = bodies(listing)
    assert len(kernels) == 30
    for name, body in kernels.items():
        loads, stores = LOADS.findall(body), STORES.findall(body)
        print(name, "loads", {k: loads.count(k) for k in set(loads)}, "stores", {k: stores.count(k) for k in set(stores)})
        assert set(loads) <= {"dwordx4", "ubyte", "dword"} and loads.count("dwordx4") >= 3 and loads.count("dword") <= 2, (name, loads)
        assert set(stores) <= {"dwordx4", "dword", "short", "byte"} and stores.count("dwordx4") >= 2, (name, stores)
        narrow = [s for s in stores if s != "dwordx4"]
        assert len(set(narrow) - {"byte"}) <= 1 and len(narrow) <= 9, (name, narrow)  # (two ends of at most two runs, the loops unrolled at most twice; the status byte)
        assert not F32_FUSED.search(body), name
