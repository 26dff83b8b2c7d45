"""The reference's own `#[test]` functions, executed under tools/rsinterp.

Everything bit-exact in this repository goes back to fixtures that tools/rsinterp produced by executing the reference's Rust text, and the
packet tests run whole reference decoders under the same interpreter.  These cases are what checks the interpreter against something
its authors did not write: each `#[test]` of the reference is a statement by the reference's authors of what their code computes, and
`cargo test` (overflow checks and debug assertions on) passes all of them.  So, per test:

  pass         it returns normally AND the interpreter counted no implicit integer wrap (Interp.overflows == 0);
  fail         RustPanic: the interpreter reads Rust differently from rustc.  Never acceptable;
  unsupported  InterpError / ParseError: syntax or std surface the interpreter lacks.  Only for Tier B, only through UNSUPPORTED below,
               and the case asserts the test STILL stops with the listed error, so the table cannot go stale or hide a later panic.

The cases are discovered from the parsed items of the reference tree (rs_harness.reference_test_functions), not from a list of names: a
test added upstream shows up as a new case, and the summary case fails until its file is put in a tier.

Tier A (must pass, no table entry): the files the fixtures, the oracle's citations and the packet tests execute, and audio/conv.rs, the
reference's own statement of its cast semantics.  Tier B (pass or listed unsupported): the container-side types the shim's look-ahead
reader handles.  Out of scope: metadata, demuxers, the AAC crate's integration test -- nothing this project executes.

Mutations (tests/golden/reference_test_mutations.json: file, line, old token, new token, sha256 of the file -- positions only, no
reference text): for at least one test per Tier A file, one token of the FUNCTION UNDER TEST is changed in memory and the reference's
test must then raise RustPanic.  A test that passed because the interpreter skipped what it asserts would not notice.
"""
import json
import time

import pytest

import rs_harness as H
from rsinterp import RustPanic
from rsinterp import interp as I
from rsinterp import parser as P

pytestmark = pytest.mark.localref

CORE = "symphonia-core/src/"
TIER_A = {  # file -> number of #[test] functions (58)
    CORE + "dsp/fft/mod.rs": 6, CORE + "dsp/mdct.rs": 1,
    "symphonia-bundle-mp3/src/layer3/hybrid_synthesis.rs": 2, "symphonia-bundle-mp3/src/synthesis.rs": 1,
    "symphonia-bundle-flac/src/decoder.rs": 1, "symphonia-bundle-flac/src/frame.rs": 1,
    "symphonia-codec-vorbis/src/codebook.rs": 4, "symphonia-codec-vorbis/src/common.rs": 2,
    "symphonia-codec-aac/src/aac/ics/mod.rs": 1,
    CORE + "io/bit.rs": 23,
    CORE + "checksum/md5.rs": 1, CORE + "checksum/crc32.rs": 1,
    CORE + "util.rs": 4,
    CORE + "audio/conv.rs": 10,
}
TIER_B = {  # (26)
    CORE + "units.rs": 5, CORE + "packet.rs": 2, CORE + "io/buf_reader.rs": 4, CORE + "io/media_source_stream.rs": 5,
    CORE + "audio/util.rs": 1, CORE + "formats/mod.rs": 1, CORE + "formats/util.rs": 1,
    "symphonia-common/src/xiph/audio/vorbis/mod.rs": 7,
}
OUT_OF_SCOPE = {  # (22) metadata 12, demuxers 9, the AAC crate's integration test 1
    "symphonia-metadata/src/embedded/vorbis.rs": 1, "symphonia-metadata/src/id3v2/frames/readers.rs": 7,
    "symphonia-metadata/src/id3v2/unsync.rs": 1, "symphonia-metadata/src/utils/base64.rs": 1, "symphonia-metadata/src/utils/std_tag.rs": 2,
    "symphonia-bundle-mp3/src/demuxer.rs": 2, "symphonia-format-caf/src/chunks.rs": 2, "symphonia-format-mkv/src/ebml.rs": 3,
    "symphonia-format-riff/src/wave/chunks.rs": 2,
    "symphonia-codec-aac/tests/tests.rs": 1,
}

# Tier B only.  test id -> (error class, a piece of the interpreter's message, why it is left).
_MSS = "std::io::Cursor and the `Box<dyn MediaSource>` it is read through are not modelled; each of these tests also pushes ~0.5 MB through the " \
       "stream one to eight bytes at a time, minutes under a tree-walking interpreter.  The shim reads packets, never a MediaSourceStream"
UNSUPPORTED = {
    CORE + "io/media_source_stream.rs::verify_mss_read": ("InterpError", "unresolved path std::io::Cursor::new", _MSS),
    CORE + "io/media_source_stream.rs::verify_mss_read_to_end": ("InterpError", "unresolved path std::io::Cursor::new", _MSS),
    CORE + "io/media_source_stream.rs::verify_mss_seek_buffered": ("InterpError", "unresolved path std::io::Cursor::new", _MSS),
    CORE + "io/media_source_stream.rs::verify_reading_be": ("InterpError", "unresolved path std::io::Cursor::new", _MSS),
    CORE + "io/media_source_stream.rs::verify_reading_le": ("InterpError", "unresolved path std::io::Cursor::new", _MSS),
    CORE + "audio/util.rs::verify_copy_from_slice_interleaved": (
        "InterpError", "no float method into_sample",
        "`impl<F, T: FromSample<F>> IntoSample<T> for F`: a blanket impl whose target type comes from the destination slice's element "
        "type, which a dynamically typed interpreter does not carry; the conversions themselves are Tier A (audio/conv.rs, 10 tests)"),
    CORE + "formats/mod.rs::verify_from_tracks_selects_longest_duration": (
        "InterpError", "unresolved path TrackFlags::empty",
        "TrackFlags comes from the third-party bitflags! macro, whose expansion is not in the reference tree"),
}

# The two fuzz tests of io/bit.rs, two allowances (both from the issue that introduced this module):
#  * `rand::rngs::SmallRng` is tests/rust/small_rng.rs, a stand-in that does not reproduce the rand crate's stream; what the tests assert
#    (`bs.buf.len() == 0` once decoding stops) must hold for any bytes;
#  * their loop runs 10 000 times upstream, far beyond a tree-walking interpreter (about 20 ms per round): that ONE literal is
#    substituted in memory by FUZZ_ROUNDS, sized to keep each test under about 20 s (400 rounds: about 9 s each).
FUZZ_TESTS = ("fuzz_bitstreamltr_read_codebook", "fuzz_bitstreamrtl_read_codebook")
FUZZ_LOOP, FUZZ_ROUNDS = "in 0..10_000 {", 400


def _fuzz_edit(text):
    assert text.count(FUZZ_LOOP) == len(FUZZ_TESTS), "the fuzz loops of io/bit.rs are not where they were"
    return text.replace(FUZZ_LOOP, "in 0..%d {" % FUZZ_ROUNDS)


FOUND = H.reference_test_functions() if H.REF.exists() else {}
IN_SCOPE = [(f, name, should_panic) for f in list(TIER_A) + list(TIER_B) for name, should_panic in FOUND.get(f, ())]
MUTATIONS = json.loads((H.ROOT / "tests" / "golden" / "reference_test_mutations.json").read_text())
RESULTS = {}  # test id -> "pass" | "unsupported"


def run_reference_test(rel, name, should_panic=False, mutation=None):
    """'pass' or ('unsupported', exception); RustPanic propagates (inverted by #[should_panic]).  Returns the interpreter too."""
    edit = _fuzz_edit if name in FUZZ_TESTS else None
    if edit is not None:
        print("%s: %d rounds instead of 10 000, SmallRng = tests/rust/small_rng.rs" % (name, FUZZ_ROUNDS))
    it = H.reference_test_interp(rel, mutation=mutation, edit=edit)
    try:
        it.call("tests::" + name)
    except RustPanic:
        if should_panic:
            return "pass", it
        raise
    except (I.InterpError, P.ParseError) as e:
        return ("unsupported", e), it
    assert not should_panic, "a #[should_panic] test returned normally"
    return "pass", it


def check_reference_test(rel, name, should_panic):
    tid = rel + "::" + name
    t0 = time.time()
    outcome, it = run_reference_test(rel, name, should_panic)
    print("%s: %s in %.1f s, %d implicit wraps" % (tid, outcome if outcome == "pass" else "unsupported (%s)" % outcome[1], time.time() - t0, it.overflows))
    if tid in UNSUPPORTED:
        assert rel in TIER_B, "only Tier B tests may be listed as unsupported"
        cls, msg, _why = UNSUPPORTED[tid]
        assert outcome != "pass", "%s passes now: take it out of UNSUPPORTED" % tid
        assert type(outcome[1]).__name__ == cls or cls == "InterpError" and isinstance(outcome[1], I.InterpError), outcome[1]
        assert msg in str(outcome[1]), "listed as %r, stops with %r" % (msg, str(outcome[1]))
        RESULTS[tid] = "unsupported"
        return
    assert outcome == "pass", "%s: %s: %s -- the interpreter lacks what this test needs" % (tid, type(outcome[1]).__name__, outcome[1])
    # cargo test builds with overflow checks: a test that passes upstream wraps nowhere implicitly
    assert it.overflows == 0, "%d implicit integer wraps where a debug build would have panicked" % it.overflows
    RESULTS[tid] = "pass"


@pytest.mark.parametrize("rel,name,should_panic", IN_SCOPE, ids=["%s::%s" % (f, n) for f, n, _ in IN_SCOPE])
def test_reference_unit_test(rel, name, should_panic):
    check_reference_test(rel, name, should_panic)


@pytest.mark.parametrize("m", MUTATIONS, ids=["%s::%s@%s:%d" % (m["test_file"], m["test"], m["file"].rsplit("/", 1)[-1], m["line"]) for m in MUTATIONS])
def test_a_mutated_function_fails_its_reference_test(m):
    """one token of the function under test changed (m["what"]): the reference's test must notice"""
    assert m["test_file"] in TIER_A
    with pytest.raises(RustPanic):
        outcome, _ = run_reference_test(m["test_file"], m["test"], mutation=m)
        pytest.fail("%s still %s with %s:%d %r -> %r" % (m["test"], outcome, m["file"], m["line"], m["old"], m["new"]))


def test_the_mutations_cover_every_tier_a_file():
    assert len(MUTATIONS) >= 12
    assert {m["test_file"] for m in MUTATIONS} == set(TIER_A)
    for m in MUTATIONS:  # the row names a test that exists, and a file that test's interpreter loads
        assert m["test"] in [n for n, _ in FOUND[m["test_file"]]], m
        assert m["file"] == m["test_file"] or m["file"] in H.REFERENCE_TEST_SIBLINGS[m["test_file"]], m


def test_summary_every_reference_test_is_accounted_for():
    """last in the module: per-tier counts, Tier A = 58 passing, and Tier A + Tier B + out of scope = every #[test] in the tree"""
    for rel, name, should_panic in IN_SCOPE:  # (cases not run in this process, e.g. under -k or xdist, are run now)
        if rel + "::" + name not in RESULTS:
            check_reference_test(rel, name, should_panic)
    tiers = {}
    for f, tests in FOUND.items():
        homes = [t for t, files in (("A", TIER_A), ("B", TIER_B), ("out of scope", OUT_OF_SCOPE)) if f in files]
        assert len(homes) == 1, "%s (%d #[test]) is in %d of the three lists" % (f, len(tests), len(homes))
        expected = (TIER_A if homes[0] == "A" else TIER_B if homes[0] == "B" else OUT_OF_SCOPE)[f]
        assert len(tests) == expected, "%s has %d #[test] functions, the list says %d" % (f, len(tests), expected)
        tiers.setdefault(homes[0], []).extend(f + "::" + n for n, _ in tests)
    for f in list(TIER_A) + list(TIER_B) + list(OUT_OF_SCOPE):
        assert f in FOUND, "%s has no #[test] any more" % f
    count = {t: {k: sum(RESULTS.get(i) == k for i in ids) for k in ("pass", "unsupported")} for t, ids in tiers.items() if t != "out of scope"}
    total = sum(len(v) for v in tiers.values())
    print("Tier A: %d pass / %d unsupported of %d" % (count["A"]["pass"], count["A"]["unsupported"], len(tiers["A"])))
    print("Tier B: %d pass / %d unsupported of %d" % (count["B"]["pass"], count["B"]["unsupported"], len(tiers["B"])))
    print("out of scope: %d; #[test] functions in the tree: %d" % (len(tiers["out of scope"]), total))
    assert len(tiers["A"]) == 58 and count["A"] == {"pass": 58, "unsupported": 0}
    assert len(tiers["B"]) == 26 and count["B"]["pass"] + count["B"]["unsupported"] == 26
    assert count["B"]["unsupported"] == len(UNSUPPORTED) and set(UNSUPPORTED) <= set(tiers["B"])
    assert len(tiers["out of scope"]) == 22
    assert total == len(tiers["A"]) + len(tiers["B"]) + len(tiers["out of scope"]) == 106
