"""The Rust side of the widening gather, as declarations: the regenerated bindings/rust/symaccel_sys.rs declares
symaccel_batcher_reserve_io, symaccel_batcher_submit_io and symaccel_host_narrow_s16 with the header's signatures (parameter names, types
and order), the generator reproduces the committed file, the ABI version is still 8, and what ctx.rs / flac.rs / alac.rs call through
`ffi::` is declared.  (The shim's code is EXECUTED against the library by tests/test_narrow_decoders.py.)"""
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
CRATE = ROOT / "bindings" / "rust" / "symphonia-accel-hip" / "src"

WANT = {
    "symaccel_batcher_reserve_io": "b: *mut SymaccelBatcher, kind: i32, param: i32, n_chains: usize, units_per_chain: usize, in_fmt: i32, out_fmt: i32, "
                                   "channels: i32, slot: *mut SymaccelBatchSlot, ticket: *mut u64",
    "symaccel_batcher_submit_io": "b: *mut SymaccelBatcher, kind: i32, param: i32, n_chains: usize, units_per_chain: usize, input: *mut *const core::ffi::c_void, "
                                  "state_io: *mut *mut core::ffi::c_void, out: *mut core::ffi::c_void, in_fmt: i32, out_fmt: i32, channels: i32, ticket: *mut u64",
    "symaccel_host_narrow_s16": "src: *const i32, dst: *mut i16, n: usize",
}


def test_symaccel_sys_declares_the_three_entry_points():
    sys_rs = (ROOT / "bindings" / "rust" / "symaccel_sys.rs").read_text()
    for fn, args in WANT.items():
        m = re.search(r"pub fn %s\((.*?)\) -> i32;" % fn, sys_rs)
        assert m, fn + " is not declared"
        assert m.group(1) == args, (fn, m.group(1))
    assert re.search(r"SYMACCEL_ABI_VERSION: \w+ = 8;", sys_rs) and re.search(r"SYMACCEL_FMT_S16: \w+ = 4;", sys_rs)
    # the fmt forms they extend are declared as ever: in_fmt is the only difference
    for fn, old in (("symaccel_batcher_reserve_io", "symaccel_batcher_reserve_fmt"), ("symaccel_batcher_submit_io", "symaccel_batcher_submit_fmt")):
        m = re.search(r"pub fn %s\((.*?)\) -> i32;" % old, sys_rs)
        assert m and m.group(1) == WANT[fn].replace("in_fmt: i32, ", ""), old


def test_the_header_says_the_same_and_the_generator_reproduces_the_file():
    import gen_rust_ffi
    text, _, funcs = gen_rust_ffi.generate()
    assert text == (ROOT / "bindings" / "rust" / "symaccel_sys.rs").read_text(), "symaccel_sys.rs is not what tools/gen_rust_ffi.py writes from the header"
    by_name = {name: (ret, params) for name, ret, params in funcs}
    for fn, args in WANT.items():
        ret, params = by_name[fn]
        assert ret == "int" and ", ".join("%s: %s" % (n, gen_rust_ffi.rust_type(t)) for n, t in params) == args, fn


def test_the_shim_calls_only_what_is_declared():
    sys_rs = (ROOT / "bindings" / "rust" / "symaccel_sys.rs").read_text()
    for mod in ("ctx.rs", "flac.rs", "alac.rs"):
        src = (CRATE / mod).read_text()
        for name in set(re.findall(r"ffi::((?:symaccel_|SYMACCEL_|Symaccel)\w+)", src)):
            assert re.search(r"\b%s\b" % name, sys_rs), "%s (%s) is not declared in symaccel_sys.rs" % (name, mod)
    ctx = (CRATE / "ctx.rs").read_text()
    assert "ffi::symaccel_batcher_reserve_io(" in ctx and "ffi::symaccel_host_narrow_s16(" in ctx
