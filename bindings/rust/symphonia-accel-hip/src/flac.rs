//! `HipFlacDecoder`: the predictor stage of every subframe (fixed and LPC, symphonia-bundle-flac/src/decoder.rs:663-752),
//! the stereo decorrelation (:32-82) and the left-justification shift (:239-242) on the MI355X.  FLAC carries no state
//! from frame to frame, so a batch is simply many frames' subframes side by side.
use std::sync::{Arc, Mutex};

use symphonia_bundle_flac::{Decorrelation, FlacDecoder, SynthBackend};
use symphonia_core::audio::{Audio, AudioBuffer, AudioMut, AudioSpec, GenericAudioBufferRef};
use symphonia_core::codecs::audio::well_known::CODEC_ID_FLAC;
use symphonia_core::codecs::audio::{AudioCodecParameters, AudioDecoder, AudioDecoderOptions, FinalizeResult, VerificationCheck};
use symphonia_core::errors::{decode_error, unsupported_error, Result};
use symphonia_core::packet::PacketRef;
use symphonia_core::support_audio_codec;

use crate::ctx::{check, narrow_words, pack_rows, place_rows, Context, Pinned, Pool, SlotCycle};
use crate::decoder::DecoderBatch;
use crate::ffi;
use crate::lookahead::{BatchCodec, Lookahead};

/// One frame after the CPU front end (frame header, subframe headers, Rice-decoded residuals: decoder.rs:381-660):
/// per channel `blocksize` words -- the warm-up samples followed by the residuals, exactly what `fixed_predict` /
/// `lpc_predict` receive --, the subframe's descriptor and quantised coefficients, and the frame's channel assignment.
pub struct ParsedFlac {
    pub blocksize: usize,
    pub words: Vec<i32>,                 // [channel][blocksize]
    pub desc: Vec<ffi::SymaccelFlacDesc>, // [channel]
    pub coeffs: Vec<i32>,                // [channel][32], bitstream order (the first coefficient multiplies the most recent sample)
    pub pair_mode: u8,                   // 0 independent, 1 left/side, 2 mid/side, 3 right/side (stereo frames only)
    pub out_shift: u32,                  // 32 - bits per sample (decoder.rs:239-242)
}

pub trait FlacFrontEnd: Send + Sync {
    /// The stream's parameters as the reference's decoder amends them from STREAMINFO (decoder.rs:110-118): sample rate,
    /// channels, bits per sample, maximum block size.
    fn params(&self) -> &AudioCodecParameters;
    fn channels(&self) -> usize;
    fn max_blocksize(&self) -> usize;
    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedFlac>;
    /// STREAMINFO's MD5 of the decoded audio, if the stream carries one (decoder.rs:118-119): what `finalize()` compares with.
    fn expected_md5(&self) -> Option<[u8; 16]> {
        None
    }
}

/// What the reference's decoder tells its `SynthBackend` about one frame (bindings/rust/patches/symphonia-bundle-flac.diff):
/// the recording backend below stores it instead of computing anything, so the decoder's `AudioBuffer` is left holding
/// every subframe's warm-up samples and residuals -- the input of the batched device call.
#[derive(Default)]
pub struct FlacRecord {
    pub desc: Vec<ffi::SymaccelFlacDesc>, // [channel]
    pub coeffs: Vec<i32>,                 // [channel][32], bitstream order
    pub pair_mode: u8,
    pub out_shift: u32,
}

impl FlacRecord {
    fn begin_frame(&mut self, nch: usize) {
        self.desc.clear();
        self.desc.resize(nch, ffi::SymaccelFlacDesc { kind: 0, order: 0, shift: 0, wasted_bits: 0 });
        self.coeffs.clear();
        self.coeffs.resize(nch * 32, 0);
        self.pair_mode = 0;
        self.out_shift = 0;
    }
}

/// The `SynthBackend` handed to the reference's `FlacDecoder`: every operation after entropy decoding is recorded, none
/// is performed.
pub struct Recorder(pub Arc<Mutex<FlacRecord>>);

impl SynthBackend for Recorder {
    fn fixed_predict(&mut self, channel: usize, order: u32, _buf: &mut [i32]) {
        let mut rec = self.0.lock().expect("flac record poisoned");
        rec.desc[channel].kind = ffi::SYMACCEL_FLAC_FIXED as u8;
        rec.desc[channel].order = order as u8;
    }

    fn lpc_predict(&mut self, channel: usize, order: u32, qlp_coeffs: &[i32; 32], qlp_coeff_shift: u32, _buf: &mut [i32]) {
        let mut rec = self.0.lock().expect("flac record poisoned");
        rec.desc[channel].kind = ffi::SYMACCEL_FLAC_LPC as u8;
        rec.desc[channel].order = order as u8;
        rec.desc[channel].shift = qlp_coeff_shift as u8;
        // the decoder stores the first coefficient it reads at index 31 (decoder.rs:477-481); the C ABI wants bitstream order
        for j in 0..order as usize {
            rec.coeffs[channel * 32 + j] = qlp_coeffs[31 - j];
        }
    }

    fn samples_shl(&mut self, channel: usize, shift: u32, _buf: &mut [i32]) {
        let mut rec = self.0.lock().expect("flac record poisoned");
        rec.desc[channel].wasted_bits = shift as u8;
    }

    fn decorrelate(&mut self, mode: Decorrelation, _plane0: &mut [i32], _plane1: &mut [i32]) {
        let mut rec = self.0.lock().expect("flac record poisoned");
        rec.pair_mode = match mode {
            Decorrelation::LeftSide => 1,
            Decorrelation::MidSide => 2,
            Decorrelation::RightSide => 3,
        };
    }

    fn left_justify(&mut self, shift: u32, _buf: &mut AudioBuffer<i32>) {
        let mut rec = self.0.lock().expect("flac record poisoned");
        rec.out_shift = shift;
    }
}

/// `FlacFrontEnd` over the reference's own decoder with the recording backend installed: frame sync, frame header, subframe
/// headers and Rice decoding are symphonia-bundle-flac's code, unmodified.
pub struct SeamFrontEnd {
    dec: FlacDecoder,
    rec: Arc<Mutex<FlacRecord>>,
    nch: usize,
    max_bs: usize,
}

impl SeamFrontEnd {
    pub fn try_new(params: &AudioCodecParameters) -> Result<Self> {
        let rec: Arc<Mutex<FlacRecord>> = Arc::new(Mutex::new(FlacRecord::default()));
        // (verification is the caller's: the MD5 would be fed the residuals)
        let opts = AudioDecoderOptions { verify: false, ..Default::default() };
        let dec = FlacDecoder::try_new_with_backend(params, &opts, Box::new(Recorder(rec.clone())))?;
        // the decoder amends its parameters from STREAMINFO (decoder.rs:110-118)
        let (Some(channels), Some(max_bs)) = (dec.codec_params().channels.clone(), dec.codec_params().max_frames_per_packet) else {
            return unsupported_error("flac: stream info is required");
        };
        Ok(SeamFrontEnd { dec, rec, nch: channels.count(), max_bs: max_bs as usize })
    }
}

impl FlacFrontEnd for SeamFrontEnd {
    fn params(&self) -> &AudioCodecParameters {
        self.dec.codec_params()
    }

    fn channels(&self) -> usize {
        self.nch
    }

    fn max_blocksize(&self) -> usize {
        self.max_bs
    }

    fn expected_md5(&self) -> Option<[u8; 16]> {
        match self.dec.codec_params().verification_check {
            Some(VerificationCheck::Md5(md5)) => Some(md5),
            _ => None,
        }
    }

    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedFlac> {
        self.rec.lock().expect("flac record poisoned").begin_frame(self.nch);
        let planes = match self.dec.decode_ref(packet)? {
            GenericAudioBufferRef::S32(planes) => planes,
            _ => return decode_error("flac: the front end's buffer is not 32-bit"),
        };
        let blocksize = planes.frames();
        let mut words = Vec::with_capacity(self.nch * blocksize);
        for c in 0..self.nch {
            match planes.plane(c) {
                Some(plane) => words.extend_from_slice(plane),
                None => return decode_error("flac: missing audio plane"),
            }
        }
        let rec = self.rec.lock().expect("flac record poisoned");
        Ok(ParsedFlac { blocksize, words, desc: rec.desc.clone(), coeffs: rec.coeffs.clone(), pair_mode: rec.pair_mode, out_shift: rec.out_shift })
    }
}

pub struct FlacBatch {
    ctx: Context,
    front: Box<dyn FlacFrontEnd>,
    nch: usize,
    words: Pinned<i32>,                 // [packet][channel][stride]
    desc: Vec<ffi::SymaccelFlacDesc>,   // [packet][channel]
    coeffs: Vec<i32>,                   // [packet][channel][32]
    // the cross-stream batcher (SYMACCEL_BATCH_FLAC_RESTORE: a chain is a subframe, units = the stream's maximum block size, so the
    // batches of every FLAC stream with that block size share launches whatever their lengths) through the slot cycle of ctx.rs: the
    // restored words of a batch that came through it are read where the device left them, in the page-locked slot
    slots: SlotCycle<FlacIndex>,
    buf: AudioBuffer<i32>,
    // Verification (`AudioDecoderOptions::verify`: the MD5 of STREAMINFO, validate.rs:25-75).  A batch through the batcher takes the
    // verify form of the kind (param 0x200 | (nch - 1) << 12: restore, then one MD5 wavefront per stream in the same launch) and comes
    // back with the state after every frame in the slot's state plane; a batch this decoder transforms itself is hashed by
    // symaccel_flac_md5 over the restored words.  `published` is the state after the last packet handed out (what `finalize` digests),
    // `chain_end` the state after the last frame of the most recently computed batch (what the next batch starts from); a seek, a skip
    // or an error drops the difference -- the reference's reset() leaves its validator alone (decoder.rs:254-256).
    verify: bool,
    replaying: bool,
    expected: Option<[u8; 16]>,
    published: ffi::SymaccelMd5State,
    chain_end: ffi::SymaccelMd5State,
    cps: Vec<ffi::SymaccelMd5State>,  // the state after every packet of a batch transformed here (a slot carries its own)
    // the batches submitted with their words as i16 (every word fits: ctx.rs narrow_words) and as i32
    narrow_batches: usize,
    wide_batches: usize,
    // the rows sent with a width of their own (SYMACCEL_NARROW_INPUT=2: ctx.rs pack_rows) at 2, 3 and 4 bytes a word
    rows_sent: [usize; 3],
}

/// Where `publish` finds a packet in its batch.
pub struct FlacIndex {
    stride: usize,     // words per subframe slot (direct: the batch's largest block size; through the batcher: the stream's)
    lens: Vec<usize>,  // block size of each packet of the batch
    modes: Vec<u8>,
    shifts: Vec<u32>,
}

const NO_DESC: ffi::SymaccelFlacDesc = ffi::SymaccelFlacDesc { kind: 0, order: 0, shift: 0, wasted_bits: 0 };

fn md5_initial() -> ffi::SymaccelMd5State {
    let mut st = ffi::SymaccelMd5State { abcd: [0; 4], len: 0, tail: [0; 64] };
    // SAFETY: a valid record; host arithmetic.
    unsafe { ffi::symaccel_md5_init(&mut st) };
    st
}

/// What the MD5 kernel needs to know of a frame: its block size, its channel assignment, and its width in bytes --
/// ceil(bits per sample / 8) (validate.rs:39-45), bits per sample being 32 - out_shift.
fn md5_frame(p: &ParsedFlac, nch: usize) -> ffi::SymaccelFlacMd5Frame {
    ffi::SymaccelFlacMd5Frame {
        block_len: p.blocksize as u16,
        pair_mode: if nch == 2 { p.pair_mode } else { 0 },
        bytes_per_sample: ((32 - p.out_shift + 7) / 8) as u8,
    }
}

impl FlacBatch {
    fn index_of(batch: &[ParsedFlac], nch: usize, stride: usize) -> FlacIndex {
        FlacIndex {
            stride,
            lens: batch.iter().map(|p| p.blocksize).collect(),
            modes: batch.iter().map(|p| if nch == 2 { p.pair_mode } else { 0 }).collect(),
            shifts: batch.iter().map(|p| p.out_shift).collect(),
        }
    }
}

impl BatchCodec for FlacBatch {
    type Parsed = ParsedFlac;

    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedFlac> {
        let p = self.front.parse(packet)?;
        if p.blocksize == 0 || p.blocksize > self.front.max_blocksize() {
            return decode_error("flac: block size outside the stream's bounds");
        }
        Ok(p)
    }

    fn transform(&mut self, batch: &[ParsedFlac]) -> Result<()> {
        // Block sizes may differ (the last frame of a stream, variable-block-size streams): every subframe gets a slot
        // of the batch's largest block size, zero-padded -- predicting the padding is harmless, it is never read back.
        let (k, nch) = (batch.len(), self.nch);
        let stride = batch.iter().map(|p| p.blocksize).max().unwrap_or(0);
        // (a batch that came through the batcher is done with: this one is published from `words`)
        self.slots.start_direct(Self::index_of(batch, nch, stride));
        let words = self.words.as_mut_slice();
        place_rows(words, batch, nch, stride, 0, |p| p.words.as_slice());
        place_rows(&mut self.desc, batch, nch, 1, NO_DESC, |p| p.desc.as_slice());
        place_rows(&mut self.coeffs, batch, nch, 32, 0, |p| p.coeffs.as_slice());
        // SAFETY: `words`, `desc` and `coeffs` cover k * nch subframes of `stride` words (sized for max_batch frames of
        // the stream's maximum block size).
        check(
            unsafe { ffi::symaccel_flac_restore(self.ctx.raw(), words.as_mut_ptr(), self.desc.as_ptr(), self.coeffs.as_ptr(), k * nch, stride) },
            self.ctx.raw(),
        )?;
        self.cps.clear();
        if self.verify && !self.replaying && k > 0 {
            // the restored words, before the decorrelation and the shift: what the reference hashes (decoder.rs:231-234)
            let frames: Vec<ffi::SymaccelFlacMd5Frame> = batch.iter().map(|p| md5_frame(p, nch)).collect();
            self.cps.resize(k, self.chain_end);
            // SAFETY: `words` holds the k * nch rows of `stride` words just restored; `frames` and `cps` have k entries.
            check(
                unsafe {
                    ffi::symaccel_flac_md5(self.ctx.raw(), words.as_ptr(), stride, frames.as_ptr(), k, nch as i32, 0, &mut self.chain_end, self.cps.as_mut_ptr())
                },
                self.ctx.raw(),
            )?;
        }
        Ok(())
    }

    fn publish(&mut self, i: usize) {
        if self.verify {
            // checkpoint i: of the slot the batch came in, or of the batch transformed here
            let slot_cp = match self.slots.parts_mut() {
                (_, Some(slot)) => Some(slot.state::<ffi::SymaccelMd5State>(0)[i]),
                _ => None,
            };
            match slot_cp {
                Some(cp) => self.published = cp,
                None => {
                    if i < self.cps.len() {
                        self.published = self.cps[i];
                    }
                }
            }
        }
        let ix = self.slots.index();
        let (n, stride, mode, shift) = (ix.lens[i], ix.stride, ix.modes[i], ix.shifts[i]);
        self.buf.clear();
        self.buf.render_uninit(Some(n));
        // the restored subframes: in the batcher's slot (zero-copy: the device wrote them there), or in this decoder's own buffer
        let words: &[i32] = self.slots.out::<i32>().unwrap_or(self.words.as_slice());
        let base = i * self.nch * stride;
        // decorrelation + left-justification of ONE frame is 2 * blocksize operations: done here on the copy out (the
        // batched device form, symaccel_flac_restore_stereo_device, is for callers that keep the PCM on the GPU)
        for c in 0..self.nch {
            if let Some(plane) = self.buf.plane_mut(c) {
                for t in 0..n {
                    let own = words[base + c * stride + t];
                    let v = if self.nch == 2 && mode != 0 {
                        let a = words[base + t];
                        let b = words[base + stride + t];
                        match (mode, c) {
                            (1, 1) => a.wrapping_sub(b),                                  // left/side: right = left - side
                            (2, _) => {
                                let mid = (a << 1) | (b & 1);                             // decoder.rs:38-73
                                if c == 0 { mid.wrapping_add(b) >> 1 } else { mid.wrapping_sub(b) >> 1 }
                            }
                            (3, 0) => a.wrapping_add(b),                                  // right/side: left = side + right
                            _ => own,
                        }
                    }
                    else {
                        own
                    };
                    plane[t] = v.wrapping_shl(shift);
                }
            }
        }
    }

    fn reset_state(&mut self) {
        self.chain_end = self.published;
    }

    fn rewind(&mut self) {
        self.chain_end = self.published;
    }

    fn set_replaying(&mut self, on: bool) {
        self.replaying = on;
    }

    fn finalize_result(&mut self) -> FinalizeResult {
        // (no digest in STREAMINFO: the reference only warns, decoder.rs:302-304)
        FinalizeResult {
            verify_ok: match (self.verify, self.expected) {
                (true, Some(expected)) => Some(self.md5_so_far() == expected),
                _ => None,
            },
        }
    }

    fn clear(&mut self) {
        self.buf.clear();
    }

    fn pooled(&self) -> bool {
        self.slots.pooled()
    }

    /// The stream's next batch goes to the process-wide batcher: the subframes are written straight into a page-locked slot; the
    /// device restores them in place, in one launch with the other streams' batches.
    fn submit(&mut self, batch: &[ParsedFlac]) -> Result<()> {
        if batch.is_empty() {
            return unsupported_error("flac: an empty batch");
        }
        let (k, nch) = (batch.len(), self.nch);
        let stride = self.front.max_blocksize(); // (the same for every batch of the stream: the group key)
        // verifying: the kind's verify form -- a frame record per packet and the state the chain starts from, entry 0 of the state plane
        let (verify, start) = (self.verify, self.chain_end);
        let param = if verify { 0x200 | ((nch as i32 - 1) << 12) } else { 0 };
        // a batch whose every warm-up sample and residual fits i16 goes up as i16 (the gather of the launch widens it); per batch
        let packed = if self.slots.narrow_input() { narrow_words(batch, |p| p.words.as_slice()) } else { None };
        // a width per row: every subframe at the narrowest of 2, 3 or 4 bytes a word that holds it, found while it is packed
        let rows = if self.slots.input_mode() == 2 { Some(pack_rows(batch, nch, |p| p.words.as_slice())) } else { None };
        let in_fmt = if rows.is_some() {
            ffi::SYMACCEL_IN_FMT_ROWS as i32
        } else if packed.is_some() {
            ffi::SYMACCEL_FMT_S16 as i32
        } else {
            0
        };
        if let Some(r) = &rows {
            for w in 0..3 {
                self.rows_sent[w] += r.counts[w];
            }
        } else if packed.is_some() {
            self.narrow_batches += 1;
        } else {
            self.wide_batches += 1;
        }
        self.slots.submit_io(ffi::SYMACCEL_BATCH_FLAC_RESTORE as i32, param, k * nch, stride, in_fmt, Self::index_of(batch, nch, stride), |slot| {
            if let Some(r) = &rows {
                r.place(slot.input::<u8>(0), stride);
                slot.input::<u8>(5).copy_from_slice(r.widths.as_slice());
            } else {
                match &packed {
                    Some(rows) => place_rows(slot.input::<i16>(0), rows, nch, stride, 0, |r| r.as_slice()),
                    None => place_rows(slot.input::<i32>(0), batch, nch, stride, 0, |p| p.words.as_slice()),
                }
            }
            place_rows(slot.input::<ffi::SymaccelFlacDesc>(1), batch, nch, 1, NO_DESC, |p| p.desc.as_slice());
            place_rows(slot.input::<i32>(2), batch, nch, 32, 0, |p| p.coeffs.as_slice());
            if verify {
                let frames = slot.input::<ffi::SymaccelFlacMd5Frame>(3);
                for (i, p) in batch.iter().enumerate() {
                    frames[i] = md5_frame(p, nch);
                }
                slot.state::<ffi::SymaccelMd5State>(0)[0] = start;
            }
            Ok(())
        })
    }

    fn collect(&mut self) -> Result<()> {
        // (verifying: entry f of the slot's state plane is the state after frame f -- `publish` reads it there)
        let mut end: Option<ffi::SymaccelMd5State> = None;
        let verify = self.verify;
        self.slots.collect(|slot| {
            if verify {
                let cps = slot.state::<ffi::SymaccelMd5State>(0);
                if !cps.is_empty() {
                    end = Some(cps[cps.len() - 1]);
                }
            }
        })?;
        if let Some(st) = end {
            self.chain_end = st;
        }
        Ok(())
    }

    fn hint(&mut self) {
        self.slots.hint();
    }

    fn abandon(&mut self) {
        self.slots.abandon();
        self.chain_end = self.published;
    }
}

impl FlacBatch {
    /// The MD5 over the packets handed out so far (the digest pads a copy: the chain goes on).
    pub fn md5_so_far(&self) -> [u8; 16] {
        let mut digest = [0u8; 16];
        // SAFETY: a valid state, room for the 16 bytes of the digest; host arithmetic.
        unsafe { ffi::symaccel_md5_digest(&self.published, digest.as_mut_ptr()) };
        digest
    }
}

impl DecoderBatch for FlacBatch {
    fn buffer(&self) -> GenericAudioBufferRef<'_> {
        self.buf.as_generic_audio_buffer_ref()
    }
}

crate::hip_decoder!(
    HipFlacDecoder,
    FlacBatch,
    ParsedFlac,
    &[support_audio_codec!(CODEC_ID_FLAC, "flac", "Free Lossless Audio Codec (MI355X predictors)")],
    "FLAC decoder with the same observable behaviour as `symphonia_bundle_flac::FlacDecoder`; with `verify` (on the cross-stream batcher) the MD5 of STREAMINFO is computed on the device and `finalize()` answers as the reference's."
);
crate::hip_decoder!(@new HipFlacDecoder, crate::frontends::flac_front_end, Box<dyn FlacFrontEnd>);

impl HipFlacDecoder {
    /// The batches this decoder sent to the batcher with their words as `i16` / as `i32`.
    pub fn narrow_batches(&self) -> usize {
        self.batch.narrow_batches
    }

    pub fn wide_batches(&self) -> usize {
        self.batch.wide_batches
    }

    /// The rows (subframes) this decoder sent with a width of their own at 2, 3 and 4 bytes a word (SYMACCEL_NARROW_INPUT=2).
    pub fn rows_sent(&self) -> [usize; 3] {
        self.batch.rows_sent
    }

    pub fn try_new_with_pool(
        _params: &AudioCodecParameters,
        opts: &AudioDecoderOptions,
        front: Box<dyn FlacFrontEnd>,
        max_batch: usize,
        pool: Option<Arc<Pool>>,
    ) -> Result<Self> {
        if opts.verify && pool.is_none() {
            // the MD5 chain (~1 us per 64-byte block per stream) is affordable only behind the batcher, where the MD5 launch of one
            // group overlaps the copies and the restore of the next on another lane: without a pool the decoder below verifies
            return unsupported_error("flac: verification needs the cross-stream batcher");
        }
        if opts.verify && front.channels() > 8 {
            return unsupported_error("flac: verification of more than 8 channels");
        }
        let params = front.params().clone();
        let (Some(rate), Some(channels)) = (params.sample_rate, params.channels.clone()) else {
            return unsupported_error("flac: sample rate and channels are required");
        };
        let nch = front.channels();
        let max_batch = max_batch.max(1);
        let max_bs = front.max_blocksize();
        let expected = if opts.verify { front.expected_md5() } else { None };
        Ok(HipFlacDecoder {
            params,
            batch: FlacBatch {
                ctx: Context::new(0)?,
                front,
                nch,
                words: Pinned::new(max_batch * nch * max_bs)?,
                desc: vec![NO_DESC; max_batch * nch],
                coeffs: vec![0; max_batch * nch * 32],
                slots: SlotCycle::new(pool, FlacBatch::index_of(&[], nch, max_bs)),
                buf: AudioBuffer::new(AudioSpec::new(rate, channels), max_bs),
                verify: opts.verify,
                replaying: false,
                expected,
                published: md5_initial(),
                chain_end: md5_initial(),
                cps: Vec::new(),
                narrow_batches: 0,
                wide_batches: 0,
                rows_sent: [0; 3],
            },
            la: Lookahead::new(max_batch),
        })
    }
}
