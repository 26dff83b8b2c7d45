"""The batcher's chunk re-basing: groups cut into many small chunks.

With the defaults (chunks of at least 8 MiB) no scenario of the suite cuts an AAC_DECODE, MP3_DECODE or VORBIS_DECODE group, so the lists
those kinds re-base per chunk (pair / filter / TNS-frame indices, unit chains, the Vorbis block offsets, kill flags, step lists and
floor classes, each relative to the chunk) were never exercised.  Here SYMACCEL_BATCH_CHUNK_MIN_KB=64 and SYMACCEL_BATCH_CHUNKS=64 are
set before the Batcher is created (the knobs are read by symaccel_batcher_create): several tickets per chunk boundary, pairs and TNS on
both sides of a boundary, a failed ticket inside a chunked group.  The scenario helpers compare every result bit for bit with the
oracle; this file adds the (launches, chunks) the batcher reports -- host arithmetic only, the same on the emulation build and the GPU.
"""
import pytest

import test_batcher as B
import test_batcher_adpcm as A
import test_batcher_kinds as K
import test_batcher_output_format as O
from emu_lib import emu_ctx  # noqa: F401

# scenario -> the (launches, chunks) of every batcher it closes
SCENARIOS = {
    "aac_decode": (lambda ctx: B.run_aac_decode(ctx, n_streams=6, frames=4, seed0=900), [(1, 6)]),
    "mp3_decode": (lambda ctx: B.run_mp3_decode(ctx, 7, 12), [(1, 4)]),
    "mp3_synth": (B.run_mp3_synth, [(1, 2)]),
    "vorbis_synth": (lambda ctx: B.run_vorbis(ctx, 8, 11, n_streams=5, nb=11), [(1, 5)]),
    "vorbis_decode": (lambda ctx: K.run_vorbis_decode(ctx, 8, 11), [(3, 5)]),
    "vorbis_decode_bad_ticket": (K.run_vorbis_decode_bad_ticket, [(1, 6)]),
    "flac": (lambda ctx: K.run_flac(ctx, 4096), [(3, 11)]),
    "alac": (lambda ctx: K.run_alac(ctx, 4096), [(3, 10)]),
    "bad_aac_blob": (K.run_bad_aac_blob, [(2, 5)]),
    "fmt_aac_synth": (lambda ctx: O.check_kind(ctx, "aac_synth"), [(1, 3), (1, 3)]),
    "fmt_aac_decode": (lambda ctx: O.check_kind(ctx, "aac_decode"), [(1, 3), (1, 3)]),
    "fmt_vorbis_synth": (lambda ctx: O.check_kind(ctx, "vorbis_synth"), [(1, 5), (1, 5)]),
    "fmt_vorbis_decode": (lambda ctx: O.check_kind(ctx, "vorbis_decode"), [(1, 5), (1, 5)]),
    "fmt_flac_restore_padded_rows": (lambda ctx: O.check_kind(ctx, "flac_restore_padded_rows"), [(1, 3), (1, 3)]),
    "adpcm_sharing": (A.check_sharing, [(6, 6)]),
    "adpcm_formats": (A.check_formats, [(10, 10)]),
}


def small_chunks(monkeypatch):
    monkeypatch.setenv("SYMACCEL_BATCH_CHUNK_MIN_KB", "64")
    monkeypatch.setenv("SYMACCEL_BATCH_CHUNKS", "64")


def run_scenario(ctx, name):
    run, want = SCENARIOS[name]
    stats = run(ctx)
    stats = list(stats) if isinstance(stats, tuple) else [stats]
    got = [(st["launches"], st["chunks"]) for st in stats]
    print(name, got)
    assert got == want, (name, got, want)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_emu_small_chunks(emu_ctx, monkeypatch, name):  # noqa: F811
    small_chunks(monkeypatch)
    run_scenario(emu_ctx, name)


def test_emu_default_chunking_has_not_moved(emu_ctx, monkeypatch):  # noqa: F811
    monkeypatch.delenv("SYMACCEL_BATCH_CHUNK_MIN_KB", raising=False)
    monkeypatch.delenv("SYMACCEL_BATCH_CHUNKS", raising=False)
    st = B.run_aac_decode(emu_ctx)
    assert st["chunks"] == st["launches"] == 1, st


@pytest.fixture(scope="module")
def gpu_ctx():
    import torch
    from symphonia_amd import Context
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    ctx = Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_gpu_small_chunks(gpu_ctx, monkeypatch):
    small_chunks(monkeypatch)
    for name in SCENARIOS:
        run_scenario(gpu_ctx, name)
