"""The batcher-slot cycle of the Rust shim -- `SlotCycle` in bindings/rust/symphonia-accel-hip/src/ctx.rs, the one owner of the page-locked
slots of the seven slot codecs -- EXECUTED on its own under tools/rsinterp, its `extern "C"` calls bound to libsymaccel (the CPU-emulation
build here, the hipcc-built library in the gpu twin), through the smallest real shape: batcher kind 10, Layer I, one chain, one packet
(tests/rust/slot_probe.rs).  The rule under test: every slot is released exactly once, on every path.  A slot that is not released stays
live in the batcher, so `slots_peak` of `Pool::stats()` -- the most slots that were ever live at once; every Harness has a pool of its own,
so it starts at 0 -- bounds the leaks: a cycle holds two slots at most (the one being handed out and the one submitted ahead).

The PCM and the state a cycle delivers are compared with `symaccel_mpa12_decode` (`Context::mpa12_decode`, mpa12.rs) of the same packet
from the same state, bit for bit."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import mpa12_ref as R  # noqa: E402
from helpers import bit_equal  # noqa: E402
from rs_harness import Harness, f32_vec, i32_vec, pool_stats, u8_vec, usize  # noqa: E402
from rsinterp import RustPanic  # noqa: E402
from rsinterp import interp as I  # noqa: E402
from test_mpa12 import case  # noqa: E402
from test_rust_adapters import LIBS  # noqa: E402

ROUNDS = 16


def u16_vec(a):
    return I.Arr([I.Int(int(x), "u16") for x in np.asarray(a).ravel()], True)


def floats(arr):
    return np.array([np.float32(x) if not isinstance(x, I.Int) else np.float32(x.v) for x in arr.a], np.float32)


class Probe:
    """A `SlotProbe` on the process-wide pool of a fresh interpreter, and a `Context` for the direct decode it is compared with."""

    def __init__(self, make_dll):
        self.h = h = Harness(make_dll())
        h.load_shim("ctx.rs", "mpa12.rs")
        h.it.load_file(ROOT / "tests" / "rust" / "slot_probe.rs")
        r = h.it.call("SlotProbe::new_pooled")
        assert r.variant == "Ok", r
        self.p = r.f["0"]
        r = h.it.call("Context::new", I.Int(0, "i32"))
        assert r.variant == "Ok", r
        self.ctx = r.f["0"]
        (codes, rec, _, _), _ = case(R.LAYER1, 1, 1)
        self.codes, self.rec = codes.ravel(), rec.ravel()  # 384 codes, a 64-byte record

    def call(self, name, *args):
        return self.h.it.call_method("SlotProbe", name, self.p, *args)

    def submit(self, tag, rec=None, fail_fill=False):
        return self.call("submit", I.Int(tag, "i64"), u16_vec(self.codes), u8_vec(self.rec if rec is None else rec), bool(fail_fill))

    def collect(self):
        return self.call("collect")

    def state(self):
        return floats(self.p.f["vvec"]), np.array([v.v for v in self.p.f["vfront"].a], np.int32)

    def out(self):
        r = self.call("out")
        return None if r.variant == "None" else floats(r.f["0"])

    def tag(self):
        return int(self.call("tag").v)

    def peak(self):
        return pool_stats(self.h)["slots_peak"]

    def direct(self, vvec, vfront):
        """(pcm, vvec, vfront) of `symaccel_mpa12_decode` on the probe's packet from the given state"""
        kind = self.h.it.resolve_value(["MpaLayer", "Layer1"], I.Env(), None)
        vv, vf, pcm, status = f32_vec(vvec), i32_vec(vfront), f32_vec(np.zeros(384, np.float32)), u8_vec(np.zeros(1, np.uint8))
        r = self.h.it.call_method("Context", "mpa12_decode", self.ctx, kind, usize(1), u16_vec(self.codes), u8_vec(self.rec), vv, vf, pcm, status)
        assert r.variant == "Ok" and status.a[0].v == 0, r
        return floats(pcm), floats(vv), np.array([v.v for v in vf.a], np.int32)

    def cycle_equals_direct(self, tag):
        """collect the pending batch: its PCM (read in the slot), the state it left and its tag == the direct decode from the state before"""
        want = self.direct(*self.state())
        r = self.collect()
        assert r.variant == "Ok", r
        vv, vf = self.state()
        assert bit_equal(self.out(), want[0]) and bit_equal(vv, want[1]) and np.array_equal(vf, want[2]) and self.tag() == tag, tag

    def two_live_slots_at_most(self):
        """submit, collect, submit: with nothing leaked before, the batcher has never seen more than two live slots"""
        assert self.submit(900).variant == "Ok"
        self.cycle_equals_direct(900)
        assert self.submit(901).variant == "Ok"
        assert self.peak() <= 2, self.peak()


@pytest.mark.parametrize("make_dll", LIBS)
def test_submit_collect_rounds_hold_two_slots_and_release_all_gives_both_back(make_dll):
    pr = Probe(make_dll)
    assert pr.out() is None and pr.tag() == -1
    for t in range(ROUNDS):
        assert pr.submit(t).variant == "Ok", t
        if t + 1 < ROUNDS:
            assert pr.collect().variant == "Ok", t
            assert pr.tag() == t
    pr.cycle_equals_direct(ROUNDS - 1)  # (the state has been carried through every round before: vvec / vfront of the read-back)
    assert pr.submit(ROUNDS).variant == "Ok"  # one handed out, one ahead
    print("slots_peak after %d rounds: %d" % (ROUNDS, pr.peak()))
    assert pr.peak() <= 2, pr.peak()  # (a slot leaked per round would make it grow with the rounds)
    pr.call("release_all")
    assert pr.out() is None
    r = pr.collect()
    assert r.variant == "Err" and r.f["0"].variant == "Unsupported", r  # nothing is pending any more
    pr.two_live_slots_at_most()  # both went back: a fresh cycle fits under the same bound


@pytest.mark.parametrize("make_dll", LIBS)
def test_submit_abandon_rounds_hold_one_slot(make_dll):
    pr = Probe(make_dll)
    before = pr.state()
    for t in range(ROUNDS):
        assert pr.submit(t).variant == "Ok", t
        pr.call("abandon")
    print("slots_peak after %d abandoned submissions: %d" % (ROUNDS, pr.peak()))
    assert pr.peak() <= 1, pr.peak()
    assert pr.out() is None and pr.tag() == -1  # nothing was ever collected: no current slot, the first index
    assert bit_equal(pr.state()[0], before[0]) and np.array_equal(pr.state()[1], before[1])  # an abandoned batch leaves the carried state alone
    assert pr.submit(ROUNDS).variant == "Ok"
    assert pr.peak() <= 1, pr.peak()
    pr.cycle_equals_direct(ROUNDS)


@pytest.mark.parametrize("make_dll", LIBS)
def test_a_failing_fill_returns_its_error_and_its_slot(make_dll):
    pr = Probe(make_dll)
    peak = pr.peak()
    r = pr.submit(1, fail_fill=True)
    assert r.variant == "Err" and r.f["0"].variant == "DecodeError", r  # the fill's own error
    r = pr.collect()
    assert r.variant == "Err" and r.f["0"].variant == "Unsupported", r  # nothing is pending
    assert pool_stats(pr.h)["pending"] == 0
    assert pr.submit(2).variant == "Ok"  # the next submit is accepted ...
    print("slots_peak before / after a failed fill and the next submit: %d / %d" % (peak, pr.peak()))
    assert pr.peak() <= peak + 1, (peak, pr.peak())  # ... into the room the failed one gave back
    pr.cycle_equals_direct(2)


@pytest.mark.parametrize("make_dll", LIBS)
def test_a_second_submit_is_refused_and_the_pending_one_collects(make_dll):
    pr = Probe(make_dll)
    assert pr.submit(1).variant == "Ok"
    peak = pr.peak()
    r = pr.submit(2)
    assert r.variant == "Err" and r.f["0"].variant == "Unsupported", r
    assert pr.peak() == peak  # (refused before a slot was reserved)
    pr.cycle_equals_direct(1)


@pytest.mark.parametrize("make_dll", LIBS)
def test_a_failing_wait_keeps_the_current_batch_and_returns_the_slot(make_dll):
    """A record whose first `bits` byte is 1 is judged on the host, in the slot (csrc/batcher.cpp check_mpa12): the ticket fails alone
    with SYMACCEL_ERR_INVALID_ARG.  `collect` ends with that error -- in the form ctx.rs `check` gives every INVALID_ARG of the library:
    the panic of the reference's assert! class, here RustPanic -- after the failed slot has gone back and with the current batch untouched."""
    pr = Probe(make_dll)
    assert pr.submit(1).variant == "Ok"
    pr.cycle_equals_direct(1)
    pcm, state = pr.out(), pr.state()
    bad = pr.rec.copy()
    bad[0] = 1
    assert pr.submit(2, rec=bad).variant == "Ok"
    with pytest.raises(RustPanic):
        pr.collect()
    assert pool_stats(pr.h)["failed_tickets"] == 1
    # the batch from before is still the current one: its index, its PCM in its slot, the state it left
    assert pr.tag() == 1 and bit_equal(pr.out(), pcm)
    assert bit_equal(pr.state()[0], state[0]) and np.array_equal(pr.state()[1], state[1])
    r = pr.collect()
    assert r.variant == "Err" and r.f["0"].variant == "Unsupported", r  # nothing is pending
    # the failed slot went back: the next submit is accepted beside the current slot, and a further round stays at two slots
    assert pr.submit(3).variant == "Ok"
    assert pr.peak() <= 2, pr.peak()
    pr.cycle_equals_direct(3)
    assert pr.submit(4).variant == "Ok"
    print("slots_peak after a failed wait and two more submissions: %d" % pr.peak())
    assert pr.peak() <= 2, pr.peak()


@pytest.mark.parametrize("make_dll", LIBS)
def test_a_direct_batch_releases_the_collected_slot(make_dll):
    pr = Probe(make_dll)
    assert pr.submit(1).variant == "Ok"
    pr.cycle_equals_direct(1)
    assert pr.out() is not None
    pr.call("start_direct", I.Int(7, "i64"))
    assert pr.out() is None and pr.tag() == 7  # served from the codec's own buffers now, under the direct batch's index
    pr.two_live_slots_at_most()  # (the collected slot still live would make it three)
