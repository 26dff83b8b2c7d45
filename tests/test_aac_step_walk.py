"""The three pieces of the AAC workgroup walk (csrc/aac.hip): the halo step, the main loop of full four-frame steps, the ragged
last step -- for every way a segment can start and end.  Frames per chain x segment length below decide how many full steps a
segment has (none, one, many), whether a ragged step follows (one, two or three frames), whether a halo frame precedes, and
where the unconditional prefetch of the main loop runs past the segment's end.  Plain chains (random legal window-sequence
walks with random shapes, as `bench.py --mix` draws them, beside an ONLY_LONG chain that keeps its window shape: the headline's
frames) and channel pairs with joint stereo on load, a non-zero incoming delay, and a second call that continues the stream
from the first call's `delay_out`: PCM and outgoing delay bit-identical to oracle.aac_synth, and the words in front of and
behind `pcm` and `delay_out` untouched.  CPU emulation here, the MI355X under `-m gpu`."""
import numpy as np
import pytest

import oracle
import test_aac_tools as T
from emu_lib import emu_ctx  # noqa: F401
from helpers import aac_sequence_chain, aac_spectra, bit_equal
from symphonia_amd import AacSpectralTools, aac_side

FRAMES = [1, 2, 3, 4, 5, 7, 8, 9, 257, 1023]
SEGMENTS = [4, 8, 12, 256]
SECOND_CALL_FRAMES = 6  # one full step and a ragged one, continuing from the first call's outgoing delay
GUARD = 512             # words in front of and behind every output buffer
GUARD_BITS = np.uint32(0x7FA5C3E1)  # (a NaN pattern no synthesis produces)


def make_case(seed, paired, frames):
    rng = np.random.default_rng(seed)
    n_pairs, extra = (1, 1) if paired else (0, 2)
    chains = 2 * n_pairs + extra
    coeffs = aac_spectra(rng, (chains, frames))
    order = rng.permutation(chains)
    pairs = np.array([[order[2 * p], order[2 * p + 1]] for p in range(n_pairs)], np.int32).reshape(n_pairs, 2)
    seqs = {c: aac_sequence_chain(rng, frames, 0.25) for c in range(chains)}
    if not paired:  # the headline's kind of chain: ONLY_LONG frames of one window shape
        seqs[0] = (np.zeros(frames, np.uint8), np.ones(frames, np.uint8), np.ones(frames, np.uint8))
    for l, r in pairs:  # the channels of a pair share their window sequence (common_window)
        seqs[int(r)] = seqs[int(l)]
    side = np.zeros((chains, frames), np.uint8)
    for c in range(chains):
        side[c] = aac_side(*seqs[c])
    desc = np.zeros((n_pairs, frames), T.oracle_dtype_js())
    for p, (l, r) in enumerate(pairs):
        for f in range(frames):
            desc[p, f] = T.js_frame(rng, short=bool(seqs[int(l)][0][f] == 2))
    delay = rng.standard_normal((chains, 1024)).astype(np.float32)  # a non-zero incoming delay line
    return coeffs, side, delay, pairs, desc


def guarded(to_dev, shape):
    """(the whole buffer on the device, the view of `shape` in its middle)"""
    n = int(np.prod(shape))
    whole = to_dev(np.full(n + 2 * GUARD, GUARD_BITS, np.uint32).view(np.float32))
    return whole, whole[GUARD:GUARD + n].reshape(shape)


def guards_intact(to_host, whole):
    bits = to_host(whole).view(np.uint32)
    return bool((bits[:GUARD] == GUARD_BITS).all() and (bits[-GUARD:] == GUARD_BITS).all())


def run(ctx, to_dev, to_host, paired, frames, seg):
    total = frames + SECOND_CALL_FRAMES
    coeffs, side, delay, pairs, desc = make_case(1000 * frames + 10 * seg + int(paired), paired, total)
    n_pairs = len(pairs)
    decoded = T.js_reference(coeffs, pairs, desc) if n_pairs else coeffs
    want_pcm, want_delay = oracle.aac_synth(decoded, side, delay)
    _, want_mid = oracle.aac_synth(decoded[:, :frames], side[:, :frames], delay)
    tools = AacSpectralTools(ctx, T.SWB_LONG, T.SWB_SHORT)
    d_pairs = to_dev(pairs) if n_pairs else None
    d_in = to_dev(delay.copy())
    ctx.set_segment(seg)
    try:
        got_pcm = []
        for lo, hi in ((0, frames), (frames, total)):
            n = hi - lo
            d_desc = to_dev(np.ascontiguousarray(desc[:, lo:hi]).view(np.uint8).reshape(n_pairs, n, 644)) if n_pairs else None
            pcm_whole, pcm = guarded(to_dev, (coeffs.shape[0], n, 1024))
            out_whole, d_out = guarded(to_dev, delay.shape)
            tools.synth_joint_stereo(to_dev(coeffs[:, lo:hi]), to_dev(side[:, lo:hi]), d_in, d_pairs, d_desc, pcm, delay_out=d_out)
            got_pcm.append(to_host(pcm))
            assert guards_intact(to_host, pcm_whole), "a store outside pcm (call %d)" % (lo > 0)
            assert guards_intact(to_host, out_whole), "a store outside delay_out (call %d)" % (lo > 0)
            if lo == 0:
                assert bit_equal(to_host(d_out), want_mid), "outgoing delay of the first call"
            d_in = d_out  # the second call continues the stream from here
    finally:
        ctx.set_segment(0)
    assert bit_equal(got_pcm[0], want_pcm[:, :frames]), "pcm of the first call"
    assert bit_equal(got_pcm[1], want_pcm[:, frames:]), "pcm of the second call"
    assert bit_equal(to_host(d_in), want_delay), "outgoing delay of the second call"


@pytest.mark.parametrize("seg", SEGMENTS)
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("paired", [False, True], ids=["plain", "paired"])
def test_emu_aac_walk_prologue_main_loop_epilogue(emu_ctx, paired, frames, seg):
    run(emu_ctx, np.ascontiguousarray, lambda a: np.array(a, copy=True), paired, frames, seg)


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests must run on an MI355X (there is no CPU path)")
    from symphonia_amd import Context
    ctx = Context(0)
    ctx.use_torch_stream()

    def to_host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()
    yield ctx, (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()), to_host
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seg", SEGMENTS)
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("paired", [False, True], ids=["plain", "paired"])
def test_gpu_aac_walk_prologue_main_loop_epilogue(gpu, paired, frames, seg):
    run(*gpu, paired, frames, seg)
