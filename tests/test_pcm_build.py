"""The access widths of the PCM conversion kernels at the ISA level: the converted samples leave in 16-byte stores.
Written as `uint4` stores, the loop that empties the LDS image was once turned by the loop vectoriser into 4-byte stores lane to lane
16 bytes apart; the source now forbids that, and this file reads the device assembly of batch_copy.hip, built with the product's flags:

  pcm_convert_kernel<src, dst>   (18) no 4-, 8- or 12-byte store at all: 16-byte stores, and byte stores for the at most 15 bytes at
                                 either end of a tile that does not start or end on a 16-byte boundary; no scratch
  batch_scatter_convert_kernel   the same for its 18 tile routines; the ONE 4-byte store it may hold is the loop of the plain copy for
                                 pieces that are 4- but not 16-byte aligned (batch_copy_kernel has the same one); no scratch
"""
import re
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tools.kernel_resources import device_asm, kernel_resources  # noqa: E402

NARROW = re.compile(r"\b(?:global|flat)_store_(?:dword|dwordx2|dwordx3)\b")
WIDE = re.compile(r"\b(?:global|flat)_store_dwordx4\b")
WIDE_LOAD = re.compile(r"\b(?:global|flat)_load_dwordx4\b")


@pytest.fixture(scope="module")
def listing():
    if not (shutil.which("hipcc") or Path("/opt/rocm/bin/hipcc").exists()):
        pytest.skip("hipcc not available")
    return device_asm("batch_copy.hip")


def bodies(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M)}


def test_the_conversion_kernels_store_sixteen_bytes_a_lane(listing):
    kernels = {n: b for n, b in bodies(listing).items() if "pcm_convert_kernel" in n}
    assert len(kernels) == 18, sorted(kernels)
    for name, body in kernels.items():
        narrow = NARROW.findall(body)
        print(name, "16-byte stores:", len(WIDE.findall(body)), "16-byte loads:", len(WIDE_LOAD.findall(body)), "narrower dword stores:", len(narrow))
        assert not narrow, "%s stores %s" % (name, sorted(set(narrow)))
        assert WIDE.findall(body) and WIDE_LOAD.findall(body), name


def test_the_converting_scatter_stores_sixteen_bytes_a_lane(listing):
    (name, body), = [(n, b) for n, b in bodies(listing).items() if "batch_scatter_convert_kernel" in n]
    narrow, wide = NARROW.findall(body), WIDE.findall(body)
    print(name, "16-byte stores:", len(wide), "narrower dword stores:", len(narrow))
    assert len(wide) >= 18 + 1, "one per tile routine and the plain copy at least: %d" % len(wide)
    assert len(narrow) <= 1 and all(n.endswith("store_dword") for n in narrow), narrow  # (the plain copy's loop for 4-byte aligned pieces)


def test_no_scratch_in_the_conversion_kernels(listing):
    res = {n: r for n, r in kernel_resources(listing).items() if "pcm_convert_kernel" in n or "batch_scatter_convert_kernel" in n}
    assert len(res) == 19
    for name, r in res.items():
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
