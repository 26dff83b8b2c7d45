"""The instruction stream of the AAC walk's main loop (csrc/aac.hip, the plain instantiation), read from the device assembly.

gfx950 counts vector loads and stores with one in-order counter, so `s_waitcnt vmcnt(0)` inside the loop means "stand still until
this frame's PCM stores are acknowledged".  The steady-state step is built so that the long arms never do that: the prefetch is
unconditional, every long arm issues exactly its four PCM stores behind it, and the prefetched lines are claimed behind those
stores -- the wait for them is vmcnt(N) with N >= 4.  Only the EIGHT_SHORT arm (global twiddle loads of the short transform) may
drain the counter."""
import re
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tools.kernel_resources import device_asm, kernel_resources  # noqa: E402

NT_STORE = re.compile(r"^\s*global_store_dwordx4\b.*\bnt\b")
VMCNT = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\((\d+)\)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):(.*)$")


@pytest.fixture(scope="module")
def plain_kernel():
    if not (shutil.which("hipcc") or Path("/opt/rocm/bin/hipcc").exists()):
        pytest.skip("hipcc not available")
    text = device_asm("aac.hip", [])
    (name,) = [k for k in kernel_resources(text) if "aac_synth_quad_kernelILb0E" in k]
    m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, flags=re.S | re.M)
    return kernel_resources(text), m.group(1).splitlines()


def blocks_of(lines):
    """[(label, header comment, [instruction lines])] in layout order; the entry block has the label ''."""
    out = [("", "", [])]
    for l in lines:
        m = LABEL.match(l)
        if m:
            out.append((m.group(1), m.group(2), []))
        elif l.strip() and (not l.lstrip().startswith(";") or ";;#ASM" in l):  # (instructions and inline-asm markers, no comments)
            out[-1][2].append(l)
    return out


def main_loop(lines):
    """The blocks (in layout order, child loops included) of the depth-1 loop that holds a block with four non-temporal PCM stores:
    a long arm's phase 2."""
    blocks = blocks_of(lines)
    found = []
    for i, (label, comment, _) in enumerate(blocks):
        if "Loop Header: Depth=1" not in comment:
            continue
        mine = "Header=%s Depth=1" % label[2:]
        last = max([j for j, b in enumerate(blocks) if mine in b[1]] + [i])
        loop = blocks[i:last + 1]
        if any(sum(bool(NT_STORE.match(l)) for l in body) == 4 for _, _, body in loop):
            found.append(loop)
    assert len(found) == 1, "expected exactly one loop with a block of four nt PCM stores, found %d" % len(found)
    return found[0]


def test_main_loop_never_drains_the_memory_counter_on_a_long_arm(plain_kernel):
    _, lines = plain_kernel
    loop = main_loop(lines)
    long_blocks = [b for b in loop if sum(bool(NT_STORE.match(l)) for l in b[2]) == 4]
    assert len(long_blocks) == 1, "one phase-2 block for the long arms"
    drains = 0
    for label, comment, body in loop:
        # the EIGHT_SHORT arm: the short transform's twiddles come from global memory (plain loads; the lines are `nt` loads) and its
        # window loops are rolled (depth-2 blocks)
        short_arm = "Depth=2" in comment or "Parent Loop" in comment or any(re.match(r"^\s*global_load_dwordx2\b(?!.*\bnt\b)", l) for l in body)
        for l in body:
            m = VMCNT.match(l)
            if m and int(m.group(1)) == 0:
                assert short_arm, "s_waitcnt vmcnt(0) outside the EIGHT_SHORT arm, in block %s: the step waits for its own PCM stores" % label
                drains += 1
    # (the short transform loads its twiddles twice: that is where the arm drains the counter)
    assert drains <= 4, drains


def test_the_wait_for_the_prefetched_lines_leaves_the_four_stores_in_flight(plain_kernel):
    _, lines = plain_kernel
    loop = main_loop(lines)
    (body,) = [b[2] for b in loop if sum(bool(NT_STORE.match(l)) for l in b[2]) == 4]
    last_store = max(i for i, l in enumerate(body) if NT_STORE.match(l))
    claim = [i for i, l in enumerate(body) if ";;#ASMSTART" in l]
    assert claim and claim[0] > last_store, "the lines are claimed behind the four PCM stores"
    waits = [int(VMCNT.match(l).group(1)) for l in body[last_store + 1:claim[0]] if VMCNT.match(l)]
    assert waits, "the claim must be where the wait for the lines is"
    assert min(waits) >= 4, "the wait for the lines also waits for PCM stores: vmcnt(%d)" % min(waits)
    # and nothing in front of the stores of this block waits for more than the side byte (eight line loads behind it)
    early = [int(VMCNT.match(l).group(1)) for l in body[:last_store] if VMCNT.match(l)]
    assert all(n >= 8 for n in early), early


def test_budget_of_the_walk(plain_kernel):
    res, _ = plain_kernel
    walks = {k: v for k, v in res.items() if "aac_synth_quad_kernel" in k}
    assert len(walks) == 2
    for name, r in walks.items():
        assert r["NumVgprs"] <= 256 and r["ScratchSize"] == 0 and r["Occupancy"] == 2, (name, r)
        assert 2 * r["LDSByteSize"] <= 160 * 1024, (name, r)  # two workgroups per CU
    plain = [r for k, r in walks.items() if "ILb0E" in k][0]
    assert plain["LDSByteSize"] == 57728  # unchanged: tables + four wave areas + one double-buffered carry
