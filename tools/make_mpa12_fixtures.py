#!/usr/bin/env python3
"""tests/golden/mpa12/*.npz: the reference's Layer I and Layer II decoders (symphonia-bundle-mp3/src/layer1/mod.rs Layer1::decode,
layer2/mod.rs Layer2::decode, with header.rs, layer12.rs and synthesis.rs) executed under tools/rsinterp on frames written by
tests/mpa12_writer.py.

    python tools/make_mpa12_fixtures.py            # (needs the reference tree) writes the fixtures
    python tools/make_mpa12_fixtures.py --check    # regenerates and compares

The fixtures hold data only:
  tables.npz   the bit patterns of FACTOR (layer1/mod.rs:19-47), LAYER12_SCALEFACTORS (layer12.rs:9-76) and of every quantisation
               class's c and d with its bits / grouping / nlevels (layer2/mod.rs:46-64), read out of the interpreter
  streams.npz  per stream: the packets, what the writer put into them in the form symaccel_mpa12_decode takes (codes, records), the
               PCM the reference decoded and its SynthesisState after the last packet
tests/mpa12_ref.py (the two dequantisations in numpy) is pinned to the reference by tests/test_mpa12.py: its PCM for the fixtures'
codes and records must be the reference's, bit for bit."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

OUT = ROOT / "tests" / "golden" / "mpa12"
CRATE = "symphonia-bundle-mp3/src/"
FILES = ("common.rs", "header.rs", "layer12.rs", "synthesis.rs", "layer1/mod.rs")
DRIVER = """
pub fn mpa12_fixture_header(data: &[u8]) -> FrameHeader { let mut r = BufReader::new(data); read_frame_header(&mut r).unwrap() }
pub fn mpa12_fixture_buffer(data: &[u8]) -> AudioBuffer<f32> { AudioBuffer::new(mpa12_fixture_header(data).spec(), 1152) }
pub fn mpa12_fixture_decode(layer: &mut dyn Layer, data: &[u8], buf: &mut AudioBuffer<f32>) -> Result<()> {
    let mut r = BufReader::new(data);
    let header = read_frame_header(&mut r)?;
    assert!(header.frame_size == r.bytes_available() as usize);
    buf.clear();
    layer.decode(&mut r, &header, buf)
}
pub fn mpa12_fixture_scalefactors() -> Vec<f32> { let mut v = Vec::new(); for i in 0..64 { v.push(LAYER12_SCALEFACTORS[i]); } v }
"""
DRIVER_L1 = """
pub fn mpa12_fixture_new() -> Layer1 { Layer1::new() }
pub fn mpa12_fixture_factor() -> Vec<f32> { let mut v = Vec::new(); for i in 0..16 { v.push(FACTOR[i]); } v }
"""
DRIVER_L2 = """
pub fn mpa12_fixture_new() -> Layer2 { Layer2::new() }
pub fn mpa12_fixture_class_f32() -> Vec<f32> { let mut v = Vec::new(); for q in QUANT_CLASS.iter() { v.push(q.c); v.push(q.d); } v }
pub fn mpa12_fixture_class_int() -> Vec<u32> {
    let mut v = Vec::new();
    for q in QUANT_CLASS.iter() { v.push(u32::from(q.bits)); v.push(u32::from(q.grouping)); v.push(u32::from(q.nlevels)); }
    v
}
"""


def interpreter(layer, src=None, before_layer=()):
    """the reference's layer decoder in an interpreter of its own (the two files define functions of the same names); `src`: another
    copy of the crate's src directory (a patched one), `before_layer`: files of it loaded in front of the layer's"""
    import rs_harness as H
    from rsinterp import Interp
    src = H.REF / CRATE if src is None else src
    it = Interp()
    for f in H.CORE_IO:
        it.load_source((H.REF / "symphonia-core/src" / f).read_text(), "symphonia-core/src/" + f)
    it.load_source(H.expand_vlc_entries((H.REF / "symphonia-core/src/io/bit.rs").read_text()), "io/bit.rs")
    it.load_file(ROOT / "tests" / "rust" / "audio_stubs.rs")
    it.globals["audio_stub_sample_mid"] = H.I.Builtin(lambda: H.I.F32(0.0), "audio_stub_sample_mid")
    for f in FILES[:-1] + tuple(before_layer) + ("layer%d/mod.rs" % layer,):
        it.load_source((src / f).read_text(), CRATE + f)
    assert not it.globals.get("__unparsed__"), it.globals.get("__unparsed__")
    it.load_source(DRIVER + (DRIVER_L1 if layer == 1 else DRIVER_L2), "mpa12_fixture_driver.rs")
    return it


def floats(arr):
    return np.array([np.float32(x) for x in arr.a], np.float32)


def state_of(dec, channels):
    """the layer's SynthesisState per channel: (v_vec f32[channels][1024], v_front i32[channels])"""
    st = dec.f["synthesis"].a[:channels]
    return (np.stack([np.concatenate([floats(row) for row in s.f["v_vec"].a]) for s in st]), np.array([s.f["v_front"].v for s in st], np.int32))


def streams():
    """(name, header, [fields of every frame]) -- the cases tests/test_mpa12.py names"""
    import mpa12_writer as W
    rng = np.random.default_rng(1152)
    out = []
    for name, h, n in (("l1_mono", W.Header(1, rate_idx=14, sr_idx=2, mode=W.MONO), 3),
                       ("l1_stereo_crc", W.Header(1, rate_idx=14, sr_idx=2, mode=W.STEREO, crc=True), 2),
                       ("l1_joint_b4", W.Header(1, rate_idx=14, sr_idx=2, mode=W.JOINT, mode_ext=0), 1),
                       ("l1_joint_b8", W.Header(1, rate_idx=13, sr_idx=0, mode=W.JOINT, mode_ext=1, padding=True), 1),
                       ("l1_joint_b12", W.Header(1, rate_idx=14, sr_idx=1, mode=W.JOINT, mode_ext=2), 1),
                       ("l1_joint_b16", W.Header(1, rate_idx=14, sr_idx=2, mode=W.JOINT, mode_ext=3, crc=True), 1),
                       ("l1_dual_m2", W.Header(1, version="2", rate_idx=14, sr_idx=2, mode=W.DUAL), 2)):
        out.append((name, h, [W.random_layer1(rng, h, scf63=(i == 0)) for i in range(n)]))
    for name, h, n in (("l2_a_stereo", W.Header(2, rate_idx=10, sr_idx=1, mode=W.STEREO), 2),
                       ("l2_b_stereo_crc", W.Header(2, rate_idx=14, sr_idx=0, mode=W.STEREO, crc=True), 2),
                       ("l2_c_mono", W.Header(2, rate_idx=2, sr_idx=0, mode=W.MONO), 2),
                       ("l2_d_mono", W.Header(2, rate_idx=2, sr_idx=2, mode=W.MONO, padding=True), 1),
                       ("l2_b_joint_b4", W.Header(2, rate_idx=14, sr_idx=2, mode=W.JOINT, mode_ext=0), 1),
                       ("l2_b_joint_b8", W.Header(2, rate_idx=14, sr_idx=2, mode=W.JOINT, mode_ext=1), 1),
                       ("l2_a_joint_b12", W.Header(2, rate_idx=14, sr_idx=1, mode=W.JOINT, mode_ext=2, crc=True), 1),
                       ("l2_b_joint_b16", W.Header(2, rate_idx=13, sr_idx=0, mode=W.JOINT, mode_ext=3), 1),
                       ("l2_m2_stereo", W.Header(2, version="2", rate_idx=14, sr_idx=0, mode=W.STEREO), 2),
                       ("l2_m2_dual", W.Header(2, version="2.5", rate_idx=13, sr_idx=2, mode=W.DUAL), 1)):
        out.append((name, h, [W.random_layer2(rng, h) for _ in range(n)]))
    return out


def generate():
    """({name: array} of tables.npz, {name: array} of streams.npz) (needs the reference tree)"""
    import mpa12_writer as W
    import rs_harness as H
    its = {1: interpreter(1), 2: interpreter(2)}
    tables = {"factor": floats(its[1].call("mpa12_fixture_factor")).view(np.uint32),
              "scalefactors": floats(its[2].call("mpa12_fixture_scalefactors")).view(np.uint32),
              "class_cd": floats(its[2].call("mpa12_fixture_class_f32")).view(np.uint32).reshape(17, 2),
              "class_bits_grouping_nlevels": np.array([x.v for x in its[2].call("mpa12_fixture_class_int").a], np.uint32).reshape(17, 3)}
    assert np.array_equal(floats(its[1].call("mpa12_fixture_scalefactors")).view(np.uint32), tables["scalefactors"])
    out, entries = {}, []
    for name, h, frames in streams():
        it = its[h.layer]
        frame, inputs = (W.layer1_frame, W.layer1_inputs) if h.layer == 1 else (W.layer2_frame, W.layer2_inputs)
        packets = np.array([np.frombuffer(frame(h, *f), np.uint8) for f in frames])
        pairs = [inputs(h, *f) for f in frames]
        dec, buf = it.call("mpa12_fixture_new"), it.call("mpa12_fixture_buffer", H.u8_vec(packets[0]))
        before = it.overflows
        pcm = np.zeros((h.channels, len(frames), 32 * h.n_frames), np.float32)
        for i, p in enumerate(packets):
            r = it.call("mpa12_fixture_decode", dec, H.u8_vec(p), buf)
            assert r.variant == "Ok", (name, i, r)
            pcm[:, i] = H.Harness.planes(buf)
        assert it.overflows == before, name
        vvec, vfront = state_of(dec, h.channels)
        out[name + "_packets"] = packets
        out[name + "_codes"] = np.stack([c for c, _ in pairs], 1)   # [channel][packet][32][n_frames]
        out[name + "_rec"] = np.stack([r for _, r in pairs], 1)     # [channel][packet][record bytes]
        out[name + "_pcm"] = pcm.view(np.uint32)                    # [channel][packet][32 * n_frames]
        out[name + "_vvec"] = vvec.view(np.uint32)                  # [channel][1024]
        out[name + "_vfront"] = vfront
        entries.append({"name": name, "layer": h.layer, "version": h.version, "channels": h.channels, "mode": h.mode, "bound": h.bound(), "crc": h.crc,
                        "bitrate": h.bitrate, "sample_rate": h.sample_rate, "packets": len(frames),
                        "alloc_table": h.alloc_table() if h.layer == 2 else None, "ref": CRATE + "layer%d/mod.rs" % h.layer})
    manifest = {"generator": "tools/make_mpa12_fixtures.py", "entries": entries, "also": [CRATE + f for f in FILES[:-1]]}
    out["manifest"] = np.frombuffer(json.dumps(manifest, indent=1, sort_keys=True).encode(), np.uint8).copy()
    return tables, out


def compare(want, have):
    return sorted(k for k in set(want) | set(have) if k not in want or k not in have or want[k].shape != have[k].shape or not np.array_equal(want[k], have[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    tables, streams_ = generate()
    if a.check:
        bad = compare(tables, dict(np.load(OUT / "tables.npz"))) + compare(streams_, dict(np.load(OUT / "streams.npz")))
        print("differs: %s" % bad if bad else "tests/golden/mpa12 matches the reference")
        raise SystemExit(1 if bad else 0)
    OUT.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT / "tables.npz", **tables)
    np.savez_compressed(OUT / "streams.npz", **streams_)
    for e in json.loads(bytes(streams_["manifest"]).decode())["entries"]:
        print("%-16s layer %d MPEG-%-3s ch %d bound %2d crc %d packets %d" % (e["name"], e["layer"], e["version"], e["channels"], e["bound"], e["crc"], e["packets"]))
    print("%s: %d bytes" % (OUT, sum(p.stat().st_size for p in OUT.glob("*.npz"))))


if __name__ == "__main__":
    main()
