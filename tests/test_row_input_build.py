"""batch_gather_widen_kernel after it learned packed 24-bit pieces: no scratch memory in the gfx950 compile of
batch_copy.hip, built with the product's flags.  The comment on batch_copy_piece_beside_tiles says what scratch costs a copy kernel.
Reads the compiler's resource record only."""
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tools.kernel_resources import device_asm, kernel_resources  # noqa: E402


@pytest.fixture(scope="module")
def resources():
    if not (shutil.which("hipcc") or Path("/opt/rocm/bin/hipcc").exists()):
        pytest.skip("hipcc not available")
    return kernel_resources(device_asm("batch_copy.hip"))


def test_no_scratch_in_the_widening_gather(resources):
    (name, r), = [(n, r) for n, r in resources.items() if "batch_gather_widen_kernel" in n]
    print(name, r)
    assert r["ScratchSize"] == 0, (name, r)


def test_the_plain_copy_kernels_have_no_scratch_either(resources):
    res = {n: r for n, r in resources.items() if "batch_copy_kernel" in n}
    assert len(res) == 4, sorted(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, (name, r)
