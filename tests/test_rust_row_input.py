"""The Rust side of a width per row (SYMACCEL_IN_FMT_ROWS).

Declarations: the regenerated bindings/rust/symaccel_sys.rs declares SYMACCEL_IN_FMT_ROWS and symaccel_host_pack_row with the header's
signature, the generator reproduces the committed file, the ABI version is still 8, and what ctx.rs / flac.rs / alac.rs call through
`ffi::` is declared.

The shim under the interpreter, on the emulation library (needs the reference tree: `localref`): written 16- and 24-bit stereo streams
from the writers of tests/test_flac_packets.py / test_alac_packets.py, decoded behind a look-ahead reader through the registry with
SYMACCEL_NARROW_INPUT=2: every packet's PCM is the reference decoder's, across the look-ahead batch boundaries and after reset(); every
batch went up through symaccel_batcher_reserve_io with in_fmt = SYMACCEL_IN_FMT_ROWS, one symaccel_host_pack_row per row, and the rows
counted per width are the rows sent; a 16-bit stream sends no row at 4 bytes and a 24-bit stream some above 2.  With
SYMACCEL_NARROW_INPUT=1 and without the variable the calls are what they were: symaccel_host_narrow_s16 and reserve_io / reserve alone."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
CRATE = ROOT / "bindings" / "rust" / "symphonia-accel-hip" / "src"
IN_FMT_ROWS = 32


def test_symaccel_sys_declares_the_new_symbols():
    sys_rs = (ROOT / "bindings" / "rust" / "symaccel_sys.rs").read_text()
    m = re.search(r"pub fn symaccel_host_pack_row\((.*?)\) -> i32;", sys_rs)
    assert m and m.group(1) == "src: *const i32, dst: *mut core::ffi::c_void, n: usize", m and m.group(1)
    assert re.search(r"SYMACCEL_IN_FMT_ROWS: \w+ = 32;", sys_rs)
    assert re.search(r"SYMACCEL_ABI_VERSION: \w+ = 8;", sys_rs)
    assert re.search(r"pub fn symaccel_host_narrow_s16\(src: \*const i32, dst: \*mut i16, n: usize\) -> i32;", sys_rs)


def test_the_header_says_the_same_and_the_generator_reproduces_the_file():
    import gen_rust_ffi
    text, _, funcs = gen_rust_ffi.generate()
    assert text == (ROOT / "bindings" / "rust" / "symaccel_sys.rs").read_text(), "symaccel_sys.rs is not what tools/gen_rust_ffi.py writes from the header"
    by_name = {name: (ret, params) for name, ret, params in funcs}
    ret, params = by_name["symaccel_host_pack_row"]
    assert ret == "int" and [n for n, _ in params] == ["src", "dst", "n"]


def test_the_shim_calls_only_what_is_declared():
    sys_rs = (ROOT / "bindings" / "rust" / "symaccel_sys.rs").read_text()
    for mod in ("ctx.rs", "flac.rs", "alac.rs"):
        src = (CRATE / mod).read_text()
        for name in set(re.findall(r"ffi::((?:symaccel_|SYMACCEL_|Symaccel)\w+)", src)):
            assert re.search(r"\b%s\b" % name, sys_rs), "%s (%s) is not declared in symaccel_sys.rs" % (name, mod)
    assert "ffi::symaccel_host_pack_row(" in (CRATE / "ctx.rs").read_text()
    for mod in ("flac.rs", "alac.rs"):
        assert "ffi::SYMACCEL_IN_FMT_ROWS" in (CRATE / mod).read_text(), mod


# ---- the shim under the interpreter ---------------------------------------------------------------------------------------------------

def shim_run(monkeypatch, codec, bps, mode):
    """one written stereo stream behind a look-ahead reader, a decoder from the registry: 8 packets (two look-ahead batches and more), a
    seek back to packet 3 with reset(), 4 packets again.  Returns (narrow batches, wide batches, rows sent, the bridge, statistics)"""
    from emu_lib import emu_library
    from rs_harness import Harness, pool_stats, registry_round_trip, usize
    from rsinterp import interp as I
    if mode:
        monkeypatch.setenv("SYMACCEL_NARROW_INPUT", str(mode))
    else:
        monkeypatch.delenv("SYMACCEL_NARROW_INPUT", raising=False)
    n, depth = 8, 4
    if codec == "flac":
        import flac_writer as W
        import test_flac_packets as T
        nch, unit = 2, 192
        ref_tree, tree = T.REF / "symphonia-bundle-flac" / "src", T.patched_tree(("symphonia-bundle-flac",)) / "symphonia-bundle-flac" / "src"
        packets, _ = W.random_stream(41, n, nch, bps, unit)
        name, cpu_name, adapter, trees = "HipFlacDecoder", "FlacDecoder", "flac.rs", dict(flac_tree=tree)
        ref = Harness(None, reference=True, flac_tree=ref_tree)
        ref_dec = T.cpu_decoder(ref, nch, bps, unit)
        params = lambda h: h.params("CODEC_ID_FLAC", extra=T.streaminfo(unit, 44100, nch, bps))  # noqa: E731
    else:
        import test_alac_packets as T
        nch, unit = 2, 128
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
            assert st == "ok" and np.array_equal(got, want[i]), (codec, bps, mode, i)

    run(0, n)
    h.it.call_method("LookaheadReader", "seek", reader, I.Int(0, "i64"), usize(3))
    h.it.call_method(name, "reset", dec)
    run(3, 4)
    nb, wb = [int(h.it.call_method(name, m, dec).v) for m in ("narrow_batches", "wide_batches")]
    rows = [int(I.deref(x).v) for x in I.seq_view(I.deref(h.it.call_method(name, "rows_sent", dec)))[0][:3]]
    return nb, wb, rows, h.bridge, pool_stats(h), nch


@pytest.mark.localref
@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("codec", ["flac", "alac"])
def test_rust_shim_sends_a_width_per_row(monkeypatch, codec, bps):
    nb, wb, rows, bridge, stats, nch = shim_run(monkeypatch, codec, bps, 2)
    calls = bridge.calls
    batches = calls.count("symaccel_batcher_reserve_io")
    assert nb == 0 and wb == 0 and batches >= 2 and calls.count("symaccel_batcher_reserve") == 0, (nb, wb, batches)
    assert all(s["in_fmt"] == IN_FMT_ROWS for n, s in bridge.scalars if n == "symaccel_batcher_reserve_io")
    assert calls.count("symaccel_host_narrow_s16") == 0
    # one symaccel_host_pack_row per row; the rows of every batch are its chains
    chains = sum(s["n_chains"] for n, s in bridge.scalars if n == "symaccel_batcher_reserve_io")
    assert sum(rows) == calls.count("symaccel_host_pack_row") == chains and chains >= batches * nch, (rows, chains)
    if bps == 16:
        assert rows[2] == 0 and rows[0] > 0, rows
    else:
        assert rows[1] + rows[2] > 0, rows
    assert stats["submissions"] == batches and stats["failed_tickets"] == 0, stats


@pytest.mark.localref
def test_rust_shim_modes_0_and_1_make_the_calls_they_made(monkeypatch):
    nb, wb, rows, bridge, stats, _ = shim_run(monkeypatch, "flac", 16, 1)
    calls = bridge.calls
    assert rows == [0, 0, 0] and calls.count("symaccel_host_pack_row") == 0
    assert wb == 0 and nb >= 2 and calls.count("symaccel_batcher_reserve_io") == nb and calls.count("symaccel_batcher_reserve") == 0, (nb, wb)
    assert all(s["in_fmt"] == 4 for n, s in bridge.scalars if n == "symaccel_batcher_reserve_io")
    assert calls.count("symaccel_host_narrow_s16") > 0 and stats["failed_tickets"] == 0
    nb, wb, rows, bridge, stats, _ = shim_run(monkeypatch, "flac", 16, 0)
    calls = bridge.calls
    assert rows == [0, 0, 0] and nb == 0 and wb >= 2, (nb, wb, rows)
    assert calls.count("symaccel_batcher_reserve") == wb and calls.count("symaccel_batcher_reserve_io") == 0
    assert calls.count("symaccel_host_pack_row") == 0 and calls.count("symaccel_host_narrow_s16") == 0 and stats["failed_tickets"] == 0
