//! `HipVorbisDecoder`: everything behind the packet decoder on the MI355X -- inverse coupling, floor-1 curve synthesis and the dot
//! product (symphonia-codec-vorbis/src/lib.rs:250-292, floor.rs:568-653), then the per-channel synthesis of every audio packet:
//! Imdct, windowing and the lapped overlap-add of `DspChannel::synth` (dsp.rs:68-145, called from lib.rs:296-331).  The front end
//! hands over residue vectors + floor posts + the coupling steps of the packet (`symaccel_vorbis_decode`); a front end that delivers
//! finished spectra (`ParsedVorbis::fused == None`; any stream with a floor of type 0) takes `symaccel_vorbis_synth`.
use std::sync::{Arc, Mutex};

use symphonia_codec_vorbis::backend::{CodedChannel, Floor1Config, SynthBackend};
use symphonia_codec_vorbis::VorbisDecoder;
use symphonia_core::audio::{Audio, AudioBuffer, AudioMut, AudioSpec, GenericAudioBufferRef};
use symphonia_core::codecs::audio::well_known::CODEC_ID_VORBIS;
use symphonia_core::codecs::audio::{AudioCodecParameters, AudioDecoder, AudioDecoderOptions};
use symphonia_core::errors::{decode_error, unsupported_error, Result};
use symphonia_core::packet::PacketRef;
use symphonia_core::support_audio_codec;

use crate::ctx::{check, Context, Pinned, Pool, SlotCycle};
use crate::decoder::DecoderBatch;
use crate::ffi;
use crate::lookahead::{BatchCodec, Lookahead};

/// One audio packet after the CPU front end (mode / window flags, floor decode, residue decode, inverse coupling and the
/// floor x residue product: lib.rs:186-292): per channel the n/2 spectral lines `DspChannel::synth` receives.
/// Channels whose floor is unused ("do not decode") carry zeros, as `synth` sees them (dsp.rs:72-75).
pub struct ParsedVorbis {
    pub trim: (usize, usize), // frames to trim from the start / end of the decoded packet (lib.rs:333-342; the decoder is gapless)
    pub long_block: bool,  // block_flag of the packet's mode (lib.rs:203-214)
    pub spectra: Vec<f32>, // [channel][n / 2], n = the block size the flag selects; with `fused`: the RESIDUE vectors
    pub fused: Option<FusedVorbis>,
}

/// What is still to be done to `ParsedVorbis::spectra` when they are the packet decoder's residue vectors (lib.rs:230-248; zeros
/// for a do-not-decode channel): the inverse coupling steps, the floor curves and the dot product (lib.rs:250-292).
pub struct FusedVorbis {
    pub floor: Vec<u8>,    // [channel]: index into `VorbisFrontEnd::floors`, or SYMACCEL_VORBIS_FLOOR_UNUSED
    pub posts: Vec<u32>,   // [channel][POSTS]: floor1_Y as read from the packet
    pub coupling: Vec<u8>, // [(magnitude channel, angle channel)], in the mapping's order
}

/// Posts per channel-block in the batch arrays (floor1_values <= 65: floor.rs:510-520).
pub const POSTS: usize = 65;

pub trait VorbisFrontEnd: Send + Sync {
    fn channels(&self) -> usize;
    /// (bs0_exp, bs1_exp) of the identification header (lib.rs:404-406)
    fn block_exps(&self) -> (i32, i32);
    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedVorbis>;
    /// The floor-1 configurations `FusedVorbis::floor` indexes (empty: this front end never returns `fused`).
    fn floors(&self) -> Vec<ffi::SymaccelVorbisFloor1Cfg>;
    /// `AudioDecoder::reset`: nothing in the Vorbis parse stage outlives a packet (the lapping state is the batch's).
    fn reset(&mut self);
}

/// What the reference's decoder hands its `SynthBackend` (bindings/rust/patches/symphonia-codec-vorbis.diff).
#[derive(Default)]
pub struct VorbisRecord {
    pub n_channels: usize,
    pub bs0_exp: i32,
    pub bs1_exp: i32,
    pub long_block: bool,
    pub spectra: Vec<f32>, // [channel][n / 2]
    pub seen: usize,
    pub floors: Vec<ffi::SymaccelVorbisFloor1Cfg>, // the fused form (configure_floors, synth_block): see FusedVorbis
    pub floor: Vec<u8>,
    pub posts: Vec<u32>,
    pub coupling: Vec<u8>,
}

/// The `SynthBackend` handed to the reference's `VorbisDecoder`: every channel's floor x residue spectrum is recorded,
/// nothing is synthesized.
pub struct Recorder(pub Arc<Mutex<VorbisRecord>>, pub bool);

impl SynthBackend for Recorder {
    fn configure(&mut self, n_channels: usize, bs0_exp: u8, bs1_exp: u8) {
        let mut rec = self.0.lock().expect("vorbis record poisoned");
        rec.n_channels = n_channels;
        rec.bs0_exp = bs0_exp as i32;
        rec.bs1_exp = bs1_exp as i32;
    }

    fn synth(&mut self, channel: usize, block_flag: bool, _prev_block_flag: bool, spectrum: &[f32], _out: &mut [f32]) {
        let mut rec = self.0.lock().expect("vorbis record poisoned");
        let half = spectrum.len();
        if rec.spectra.len() != rec.n_channels * half {
            rec.spectra.clear();
            rec.spectra.resize(rec.n_channels * half, 0.0);
        }
        rec.long_block = block_flag;
        rec.spectra[channel * half..(channel + 1) * half].copy_from_slice(spectrum);
        rec.seen += 1;
    }

    fn reset(&mut self) {}

    /// `Recorder(_, true)`: take the blocks in front of the inverse coupling (the second seam of the patch).
    fn takes_blocks(&self) -> bool {
        self.1
    }

    fn configure_floors(&mut self, floors: &[Option<Floor1Config>]) {
        let mut rec = self.0.lock().expect("vorbis record poisoned");
        rec.floors.clear();
        for f in floors.iter() {
            let mut cfg = ffi::SymaccelVorbisFloor1Cfg { multiplier: 1, n_posts: 0, pad: [0; 2], x_list: [0; 65] };
            if let Some(f) = f {
                cfg.multiplier = f.multiplier;
                cfg.n_posts = f.x_list.len().min(POSTS) as u8;
                for (dst, x) in cfg.x_list.iter_mut().zip(f.x_list.iter()) {
                    *dst = *x;
                }
            }
            rec.floors.push(cfg);
        }
    }

    fn synth_block(&mut self, block_flag: bool, _prev_block_flag: bool, couplings: &[(u8, u8)], channels: &[CodedChannel<'_>], _out: &mut AudioBuffer<f32>) {
        let mut rec = self.0.lock().expect("vorbis record poisoned");
        let nch = rec.n_channels;
        let half = channels.first().map(|c| c.residue.len()).unwrap_or(0);
        rec.long_block = block_flag;
        rec.spectra.clear();
        rec.spectra.resize(nch * half, 0.0);
        rec.floor.clear();
        rec.floor.resize(nch, ffi::SYMACCEL_VORBIS_FLOOR_UNUSED as u8);
        rec.posts.clear();
        rec.posts.resize(nch * POSTS, 0);
        rec.coupling.clear();
        for ch in channels.iter() {
            let c = ch.plane;
            if c >= nch {
                continue;
            }
            // a do-not-decode channel's residue buffer is stale (residue.rs:253-259 returns before touching it): its spectrum is 0
            if !ch.do_not_decode {
                rec.spectra[c * half..(c + 1) * half].copy_from_slice(ch.residue);
            }
            if let Some((index, posts)) = ch.floor {
                rec.floor[c] = index as u8;
                for (dst, y) in rec.posts[c * POSTS..(c + 1) * POSTS].iter_mut().zip(posts.iter()) {
                    *dst = *y;
                }
            }
            rec.seen += 1;
        }
        // the steps name channels by their position in `channels`: the batch keeps channels by audio plane
        for (m, a) in couplings.iter() {
            if let (Some(mc), Some(ac)) = (channels.get(*m as usize), channels.get(*a as usize)) {
                rec.coupling.push(mc.plane as u8);
                rec.coupling.push(ac.plane as u8);
            }
        }
    }
}

/// `VorbisFrontEnd` over the reference's own decoder with the recording backend installed: setup headers, codebooks, floor
/// and residue decoding are symphonia-codec-vorbis's code, unmodified.  `fused` (the default, for streams whose floors are all of
/// type 1) stops there -- the recorder takes the blocks in front of the inverse coupling and `parse` returns residue vectors + posts
/// + coupling steps (`ParsedVorbis::fused`); without it the reference's coupling, floor synthesis and dot product run too.
pub struct SeamFrontEnd {
    dec: VorbisDecoder,
    rec: Arc<Mutex<VorbisRecord>>,
}

impl SeamFrontEnd {
    pub fn try_new(params: &AudioCodecParameters, opts: &AudioDecoderOptions) -> Result<Self> {
        Self::try_new_at(params, opts, true)
    }

    /// `fused == false`: the first-generation seam (behind the dot product).
    pub fn try_new_at(params: &AudioCodecParameters, _opts: &AudioDecoderOptions, fused: bool) -> Result<Self> {
        let rec: Arc<Mutex<VorbisRecord>> = Arc::new(Mutex::new(VorbisRecord::default()));
        // the front end never silences or trims: both are applied to what the device produced (VorbisBatch::publish)
        let opts = AudioDecoderOptions { gapless: false, ..Default::default() };
        let dec = VorbisDecoder::try_new_with_backend(params, &opts, Box::new(Recorder(rec.clone(), fused)))?;
        Ok(SeamFrontEnd { dec, rec })
    }
}

impl VorbisFrontEnd for SeamFrontEnd {
    fn channels(&self) -> usize {
        self.rec.lock().expect("vorbis record poisoned").n_channels
    }

    fn block_exps(&self) -> (i32, i32) {
        let rec = self.rec.lock().expect("vorbis record poisoned");
        (rec.bs0_exp, rec.bs1_exp)
    }

    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedVorbis> {
        self.rec.lock().expect("vorbis record poisoned").seen = 0;
        self.dec.decode_ref(packet)?;
        let rec = self.rec.lock().expect("vorbis record poisoned");
        if rec.seen != rec.n_channels {
            return decode_error("vorbis: the packet did not reach the synthesis stage for every channel");
        }
        // (the decoder hands blocks over only if the recorder takes them AND every floor is of type 1: then `floors` is filled)
        let fused = if rec.floors.is_empty() {
            None
        }
        else {
            Some(FusedVorbis { floor: rec.floor.clone(), posts: rec.posts.clone(), coupling: rec.coupling.clone() })
        };
        Ok(ParsedVorbis {
            trim: (packet.trim_start.get() as usize, packet.trim_end.get() as usize),
            long_block: rec.long_block,
            spectra: rec.spectra.clone(),
            fused,
        })
    }

    fn floors(&self) -> Vec<ffi::SymaccelVorbisFloor1Cfg> {
        self.rec.lock().expect("vorbis record poisoned").floors.clone()
    }

    fn reset(&mut self) {
        // VorbisDecoder::reset (lib.rs:367-374): Dsp::reset -- the reference's own lapping state, which the recording backend
        // never reads -- kept in step anyway
        self.dec.reset();
    }
}

pub struct VorbisBatch {
    ctx: Context,
    front: Box<dyn VorbisFrontEnd>,
    nch: usize,
    bs: [usize; 2],           // block sizes of flag 0 / 1
    spectra: Pinned<f32>,     // [channel][packed lines of the batch]
    flags: Vec<u8>,           // [channel][packet] (the same flag for every channel of a packet)
    prev_flag: Vec<i32>,      // [channel]: -1 = no previous block (after reset), else the last block's flag
    overlap: Vec<f32>,        // [channel][bs1 / 2]
    pcm: Pinned<f32>,         // [channel][packed samples of the batch]
    floors: Vec<ffi::SymaccelVorbisFloor1Cfg>, // the fused form: the stream's floor-1 configurations,
    floor: Vec<u8>,           //   [channel][packet] floor index or SYMACCEL_VORBIS_FLOOR_UNUSED,
    posts: Vec<u32>,          //   [channel][packet][POSTS]
    // the cross-stream batcher (SYMACCEL_BATCH_VORBIS_DECODE for a front end that hands on residue + posts, SYMACCEL_BATCH_VORBIS_SYNTH for
    // one that hands on spectra) through the slot cycle of ctx.rs: every chain's planes at their largest -- max_batch x bs1 / 2 --, the
    // packed data at the front, so that streams with different block flags share a launch.  The PCM of a batch that came through it is
    // read where the device left it; `floor_index` = what the batcher calls this stream's floor configurations.
    slots: SlotCycle<VorbisIndex>,
    floor_index: Vec<u8>,
    buf: AudioBuffer<f32>,
}

/// Where `publish` finds a packet in its batch.
pub struct VorbisIndex {
    pcm_stride: usize,           // samples of a channel's PCM plane (direct: the packed samples of the batch; through the batcher: the plane at its largest)
    pcm_off: Vec<usize>,         // per packet of the batch: offset of its samples in a channel's PCM; one extra = total
    emits: Vec<bool>,            // per packet: false for the first block after a reset (lib.rs:335-338: silenced when gapless)
    trims: Vec<(usize, usize)>,  // per packet of the batch
}

/// The writers below give a batch the ONE layout `symaccel_vorbis_decode` / `symaccel_vorbis_synth` and the batcher's slot share, into
/// whichever planes they are handed.  Two things remain apart on purpose: the pitch of a chain's spectrum plane (the packed lines of the
/// batch in this decoder's own buffer, the plane at its largest in the slot -- a parameter of `place_spectra`), and the coupling steps
/// (two host arrays for the direct call, one blob plane in the slot: `coupling_of` makes the arrays, the blob is written in `submit`).
impl VorbisBatch {
    /// The packed layout of a batch inside a chain (include/symaccel.h, "Vorbis"): block b owns n_b / 2 lines and (prev_n + n_b) / 4
    /// samples; a first block without a previous one owns n_b / 2 sample slots and leaves them untouched.  Returns the offset of every
    /// packet's lines, the lines of the batch, and the index (`pcm_stride` = the samples of the batch).
    fn pack(bs: &[usize; 2], prev_flag: i32, batch: &[ParsedVorbis]) -> (Vec<usize>, usize, VorbisIndex) {
        let mut prev = prev_flag;
        let (mut lines, mut samples) = (0usize, 0usize);
        let mut spec_off = Vec::with_capacity(batch.len());
        let mut index = VorbisIndex { pcm_stride: 0, pcm_off: Vec::with_capacity(batch.len() + 1), emits: Vec::with_capacity(batch.len()), trims: Vec::with_capacity(batch.len()) };
        for p in batch {
            let n = bs[p.long_block as usize];
            spec_off.push(lines);
            index.pcm_off.push(samples);
            index.emits.push(prev >= 0);
            index.trims.push(p.trim);
            lines += n / 2;
            samples += if prev >= 0 { (bs[prev as usize] + n) / 4 } else { n / 2 };
            prev = p.long_block as i32;
        }
        index.pcm_off.push(samples);
        index.pcm_stride = samples;
        (spec_off, lines, index)
    }

    /// [channel][packed lines]: a chain's plane is `pitch` lines
    fn place_spectra(dst: &mut [f32], batch: &[ParsedVorbis], bs: &[usize; 2], nch: usize, pitch: usize, spec_off: &[usize]) {
        for (i, p) in batch.iter().enumerate() {
            let half = bs[p.long_block as usize] / 2;
            for c in 0..nch {
                let at = c * pitch + spec_off[i];
                dst[at..at + half].copy_from_slice(&p.spectra[c * half..(c + 1) * half]);
            }
        }
    }

    /// [channel][packet]
    fn place_flags(dst: &mut [u8], batch: &[ParsedVorbis], nch: usize) {
        let k = batch.len();
        for (i, p) in batch.iter().enumerate() {
            for c in 0..nch {
                dst[c * k + i] = p.long_block as u8;
            }
        }
    }

    /// [channel][packet]: the floor of every channel-block under the number `name` gives the stream's own
    fn place_floor(dst: &mut [u8], batch: &[ParsedVorbis], nch: usize, name: impl Fn(u8) -> u8) {
        let k = batch.len();
        for (i, p) in batch.iter().enumerate() {
            let Some(f) = &p.fused else { continue };
            for c in 0..nch {
                dst[c * k + i] = name(f.floor[c]);
            }
        }
    }

    /// [channel][packet][POSTS]
    fn place_posts(dst: &mut [u32], batch: &[ParsedVorbis], nch: usize) {
        let k = batch.len();
        for (i, p) in batch.iter().enumerate() {
            let Some(f) = &p.fused else { continue };
            for c in 0..nch {
                let at = (c * k + i) * POSTS;
                dst[at..at + POSTS].copy_from_slice(&f.posts[c * POSTS..(c + 1) * POSTS]);
            }
        }
    }

    /// The (magnitude, angle) pairs of the batch back to back, and the index of every packet's first step; one extra = total.
    fn coupling_of(batch: &[ParsedVorbis]) -> (Vec<u8>, Vec<u32>) {
        let mut steps: Vec<u8> = Vec::new();
        let mut first: Vec<u32> = Vec::with_capacity(batch.len() + 1);
        first.push(0);
        for p in batch {
            let Some(f) = &p.fused else { continue };
            steps.extend_from_slice(&f.coupling);
            first.push((steps.len() / 2) as u32);
        }
        (steps, first)
    }
}

impl BatchCodec for VorbisBatch {
    type Parsed = ParsedVorbis;

    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedVorbis> {
        self.front.parse(packet)
    }

    fn transform(&mut self, batch: &[ParsedVorbis]) -> Result<()> {
        let (k, nch) = (batch.len(), self.nch);
        let (spec_off, lines, index) = Self::pack(&self.bs, self.prev_flag[0], batch);
        let samples = index.pcm_stride;
        // (a batch that came through the batcher is done with: this one is published from `pcm`)
        self.slots.start_direct(index);
        Self::place_spectra(self.spectra.as_mut_slice(), batch, &self.bs, nch, lines, &spec_off);
        Self::place_flags(&mut self.flags, batch, nch);
        let (bs0_exp, bs1_exp) = self.front.block_exps();
        if k > 0 && batch.iter().all(|p| p.fused.is_some()) {
            return self.transform_fused(batch, lines, samples);
        }
        // SAFETY: the buffers cover nch chains of `lines` / `samples` / `k` elements (sized for max_batch long blocks).
        check(
            unsafe {
                ffi::symaccel_vorbis_synth(
                    self.ctx.raw(),
                    bs0_exp,
                    bs1_exp,
                    self.spectra.as_slice().as_ptr(),
                    lines,
                    self.flags.as_ptr(),
                    self.prev_flag.as_mut_ptr(),
                    self.overlap.as_mut_ptr(),
                    self.pcm.as_mut_slice().as_mut_ptr(),
                    samples,
                    self.nch,
                    k,
                )
            },
            self.ctx.raw(),
        )
    }

    fn publish(&mut self, i: usize) {
        let ix = self.slots.index();
        let frames = if ix.emits[i] { ix.pcm_off[i + 1] - ix.pcm_off[i] } else { 0 };
        self.buf.clear();
        self.buf.render_uninit(Some(frames));
        // the batch's PCM: in the batcher's slot (zero-copy: the device wrote it there), or in this decoder's own buffer
        let pcm: &[f32] = self.slots.out::<f32>().unwrap_or(self.pcm.as_slice());
        for c in 0..self.nch {
            let src = c * ix.pcm_stride + ix.pcm_off[i];
            if let Some(plane) = self.buf.plane_mut(c) {
                plane[..frames].copy_from_slice(&pcm[src..src + frames]);
            }
        }
        // lib.rs:333-342 (gapless): the first packet after a reset is silenced (`emits`), every other one is trimmed
        if ix.emits[i] {
            self.buf.trim(ix.trims[i].0, ix.trims[i].1);
        }
    }

    fn reset_state(&mut self) {
        self.front.reset();
        // Dsp::reset (dsp.rs:45-56): lapping state empty, overlap zeroed
        self.prev_flag.fill(-1);
        self.overlap.fill(0.0);
    }

    fn clear(&mut self) {
        self.buf.clear();
    }

    fn pooled(&self) -> bool {
        self.slots.pooled()
    }

    /// The stream's next batch goes to the process-wide batcher: residue (or spectra), flags, floor indices, posts and the coupling steps
    /// are written straight into a page-locked slot; coupling, floor curves, dot product and synthesis run in one launch with the other
    /// streams' batches (lib.rs:250-331).
    fn submit(&mut self, batch: &[ParsedVorbis]) -> Result<()> {
        if batch.is_empty() {
            return unsupported_error("vorbis: an empty batch");
        }
        let (k, nch) = (batch.len(), self.nch);
        let fused = batch.iter().all(|p| p.fused.is_some());
        if !fused && batch.iter().any(|p| p.fused.is_some()) {
            return unsupported_error("vorbis: a batch is all residue + posts, or all spectra");
        }
        let (bs0_exp, bs1_exp) = self.front.block_exps();
        let cap = k * self.bs[1] / 2; // a chain's spectrum / PCM plane at its largest
        let (spec_off, _, mut index) = Self::pack(&self.bs, self.prev_flag[0], batch);
        index.pcm_stride = cap;
        let (kind, param) = if fused {
            (ffi::SYMACCEL_BATCH_VORBIS_DECODE as i32, bs0_exp | (bs1_exp << 8) | ((nch as i32) << 16))
        }
        else {
            (ffi::SYMACCEL_BATCH_VORBIS_SYNTH as i32, bs0_exp | (bs1_exp << 8))
        };
        self.slots.submit(kind, param, nch, k, index, |slot| {
            Self::place_spectra(slot.input::<f32>(0), batch, &self.bs, nch, cap, &spec_off);
            Self::place_flags(slot.input::<u8>(1), batch, nch);
            if fused {
                // (the stream's floor numbers become the batcher's: registered when the decoder was built)
                Self::place_floor(slot.input::<u8>(2), batch, nch, |local| {
                    if (local as usize) < self.floor_index.len() { self.floor_index[local as usize] } else { ffi::SYMACCEL_VORBIS_FLOOR_UNUSED as u8 }
                });
                Self::place_posts(slot.input::<u32>(3), batch, nch);
                // the coupling blob: first[k + 1] u32 (little endian), padded to 16 bytes, then the (magnitude, angle) pairs
                let (steps, first) = Self::coupling_of(batch);
                let blob = slot.input::<u8>(4);
                let steps_at = ((k + 1) * 4 + 15) & !15;
                if steps_at + steps.len() > blob.len() {
                    return unsupported_error("vorbis: more coupling steps than a batcher submission holds");
                }
                for (b, v) in first.iter().enumerate() {
                    blob[4 * b..4 * b + 4].copy_from_slice(&v.to_le_bytes());
                }
                blob[steps_at..steps_at + steps.len()].copy_from_slice(&steps);
            }
            slot.state::<i32>(0).copy_from_slice(&self.prev_flag);
            slot.state::<f32>(1).copy_from_slice(&self.overlap);
            Ok(())
        })
    }

    fn collect(&mut self) -> Result<()> {
        // the lapping state after the batch; the PCM stays where it is
        self.slots.collect(|slot| {
            self.prev_flag.copy_from_slice(slot.state::<i32>(0));
            self.overlap.copy_from_slice(slot.state::<f32>(1));
        })
    }

    fn hint(&mut self) {
        self.slots.hint();
    }

    fn abandon(&mut self) {
        self.slots.abandon();
    }
}

impl VorbisBatch {
    /// lib.rs:250-331 for the whole batch in one call: inverse coupling, floor curves, dot product and synthesis on the device from
    /// the packet decoder's residue vectors (already packed into `spectra` by `transform`) and posts.
    fn transform_fused(&mut self, batch: &[ParsedVorbis], lines: usize, samples: usize) -> Result<()> {
        let k = batch.len();
        Self::place_floor(&mut self.floor, batch, self.nch, |local| local);
        Self::place_posts(&mut self.posts, batch, self.nch);
        let (coupling, first) = Self::coupling_of(batch);
        let (bs0_exp, bs1_exp) = self.front.block_exps();
        // SAFETY: residue / flags / floor / posts / pcm cover nch chains of `lines` / k / k / k * POSTS / `samples` elements (sized for
        // max_batch long blocks), `first` k + 1 entries, `coupling` two bytes per step; null stands for an empty step list.  The
        // call returns after the PCM and the updated state are back in host memory.
        check(
            unsafe {
                ffi::symaccel_vorbis_decode(
                    self.ctx.raw(),
                    bs0_exp,
                    bs1_exp,
                    self.spectra.as_slice().as_ptr(),
                    lines,
                    self.flags.as_ptr(),
                    self.floor.as_ptr(),
                    self.posts.as_ptr(),
                    POSTS,
                    self.floors.as_ptr(),
                    self.floors.len(),
                    self.nch,
                    if coupling.is_empty() { std::ptr::null() } else { coupling.as_ptr() },
                    first.as_ptr(),
                    self.prev_flag.as_mut_ptr(),
                    self.overlap.as_mut_ptr(),
                    self.pcm.as_mut_slice().as_mut_ptr(),
                    samples,
                    self.nch,
                    k,
                )
            },
            self.ctx.raw(),
        )
    }
}

impl DecoderBatch for VorbisBatch {
    fn buffer(&self) -> GenericAudioBufferRef<'_> {
        self.buf.as_generic_audio_buffer_ref()
    }
}

crate::hip_decoder!(
    HipVorbisDecoder,
    VorbisBatch,
    ParsedVorbis,
    &[support_audio_codec!(CODEC_ID_VORBIS, "vorbis", "Vorbis (MI355X synthesis)")],
    "Vorbis decoder with the same observable behaviour as `symphonia_codec_vorbis::VorbisDecoder`."
);
crate::hip_decoder!(@new HipVorbisDecoder, crate::frontends::vorbis_front_end, Box<dyn VorbisFrontEnd>);

impl HipVorbisDecoder {
    pub fn try_new_with_pool(
        params: &AudioCodecParameters,
        opts: &AudioDecoderOptions,
        front: Box<dyn VorbisFrontEnd>,
        max_batch: usize,
        pool: Option<Arc<Pool>>,
    ) -> Result<Self> {
        if !opts.gapless {
            // Without gapless support the reference returns the first block after a reset windowed against silence
            // (lib.rs:316-331 with an all-zero overlap); the batched call does not compute that half block.  The decoder
            // registered below this one takes such tracks (fallback.rs).
            return unsupported_error("vorbis: the batched decoder implements the gapless (default) behaviour only");
        }
        let (Some(rate), Some(channels)) = (params.sample_rate, params.channels.clone()) else {
            return unsupported_error("vorbis: sample rate and channels are required");
        };
        let nch = front.channels();
        let max_batch = max_batch.max(1);
        let (bs0_exp, bs1_exp) = front.block_exps();
        let bs = [1usize << bs0_exp, 1usize << bs1_exp];
        let floors = front.floors();
        // the stream's floor-1 configurations under the batcher's numbers (a setup entry that is no floor 1 has no posts to render: unused);
        // a batcher that has no room for them (255 distinct configurations) leaves this stream batching on its own
        let mut pool = pool;
        let mut floor_index: Vec<u8> = Vec::with_capacity(floors.len());
        if let Some(p) = pool.clone() {
            for cfg in floors.iter() {
                if cfg.n_posts < 2 {
                    floor_index.push(ffi::SYMACCEL_VORBIS_FLOOR_UNUSED as u8);
                    continue;
                }
                match p.vorbis_floor(cfg) {
                    Ok(index) => floor_index.push(index),
                    Err(_) => {
                        pool = None;
                        break;
                    }
                }
            }
        }
        Ok(HipVorbisDecoder {
            params: params.clone(),
            batch: VorbisBatch {
                ctx: Context::new(0)?,
                front,
                nch,
                bs,
                spectra: Pinned::new(nch * max_batch * bs[1] / 2)?,
                flags: vec![0; nch * max_batch],
                prev_flag: vec![-1; nch],
                overlap: vec![0.0; nch * bs[1] / 2],
                pcm: Pinned::new(nch * max_batch * bs[1] / 2)?,
                floors,
                floor: vec![0; nch * max_batch],
                posts: vec![0; nch * max_batch * POSTS],
                slots: SlotCycle::new(pool, VorbisBatch::pack(&bs, -1, &[]).2),
                floor_index,
                buf: AudioBuffer::new(AudioSpec::new(rate, channels), bs[1] / 2),
            },
            la: Lookahead::new(max_batch),
        })
    }
}
