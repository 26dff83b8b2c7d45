//! `HipAlacDecoder`: the adaptive predictor of every element channel (symphonia-codec-alac/src/lib.rs:165-264) on the MI355X;
//! the mid-side decorrelation (:664-671), the separately coded low bits (:574-598) and the left-justification (:409-414) of ONE
//! packet are a few operations per sample and happen on the copy out.  ALAC carries no state from packet to packet, so a batch
//! is simply many packets' element channels side by side.
use std::sync::{Arc, Mutex};

use symphonia_codec_alac::{AlacDecoder, Prediction, SynthBackend};
use symphonia_common::apple::audio::alac::MagicCookie;
use symphonia_core::audio::{Audio, AudioBuffer, AudioMut, AudioSpec, GenericAudioBufferRef};
use symphonia_core::codecs::audio::well_known::CODEC_ID_ALAC;
use symphonia_core::codecs::audio::{AudioCodecParameters, AudioDecoder, AudioDecoderOptions};
use symphonia_core::errors::{decode_error, unsupported_error, Result};
use symphonia_core::packet::PacketRef;
use symphonia_core::support_audio_codec;

use crate::ctx::{check, narrow_words, pack_rows, place_rows, Context, Pinned, Pool, SlotCycle};
use crate::decoder::DecoderBatch;
use crate::ffi;
use crate::lookahead::{BatchCodec, Lookahead};

/// The mid-side parameters of one channel pair element (lib.rs:541-560).
#[derive(Clone, Copy)]
pub struct AlacPair {
    pub plane0: usize,
    pub plane1: usize,
    pub weight: i32,
    pub shift: u8,
}

/// The separately coded low bits of one element (lib.rs:531-539, 574-598); interleaved for a channel pair.
#[derive(Clone)]
pub struct AlacTail {
    pub plane0: usize,
    pub plane1: Option<usize>,
    pub shift: u8,
    pub bits: Vec<u16>,
}

/// One packet after the CPU front end (element headers, adaptive Golomb-Rice decoding: lib.rs:83-163, 470-539): per plane
/// `frames` words -- the residuals of a compressed element, or the samples of an uncompressed one (predictor order 0) --, the
/// element channel's predictor, and what follows the predictor.
pub struct ParsedAlac {
    pub frames: usize,
    pub words: Vec<i32>,                 // [plane][frames]
    pub desc: Vec<ffi::SymaccelAlacDesc>, // [plane]
    pub coeffs: Vec<i32>,                // [plane][32]
    pub pairs: Vec<AlacPair>,
    pub tails: Vec<AlacTail>,
    pub out_shift: u32,                  // 32 - bit depth
}

pub trait AlacFrontEnd: Send + Sync {
    /// The stream's parameters as the reference's decoder amends them from the magic cookie (lib.rs:305-308).
    fn params(&self) -> &AudioCodecParameters;
    fn channels(&self) -> usize;
    fn max_frames(&self) -> usize;
    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedAlac>;
}

/// What the reference's decoder tells its `SynthBackend` about one packet (bindings/rust/patches/symphonia-codec-alac.diff): the
/// recording backend below stores it instead of computing anything, so the decoder's `AudioBuffer` is left holding every element
/// channel's residuals -- the input of the batched device call.
#[derive(Default)]
pub struct AlacRecord {
    pub desc: Vec<ffi::SymaccelAlacDesc>,
    pub coeffs: Vec<i32>,
    pub pairs: Vec<AlacPair>,
    pub tails: Vec<AlacTail>,
    pub out_shift: u32,
}

impl AlacRecord {
    fn begin_packet(&mut self, nch: usize) {
        self.desc.clear();
        // (order 0: no prediction -- planes of uncompressed elements, and planes the packet does not code, stay as they are)
        self.desc.resize(nch, ffi::SymaccelAlacDesc { mode: 0, lpc_order: 0, shift: 0, bps: 32 });
        self.coeffs.clear();
        self.coeffs.resize(nch * 32, 0);
        self.pairs.clear();
        self.tails.clear();
        self.out_shift = 0;
    }
}

/// The `SynthBackend` handed to the reference's `AlacDecoder`: every operation after entropy decoding is recorded, none is
/// performed.
pub struct Recorder(pub Arc<Mutex<AlacRecord>>);

impl SynthBackend for Recorder {
    fn predict(&mut self, channel: usize, pred: &Prediction, _out: &mut [i32]) -> Result<()> {
        // lib.rs:167-169: the check the predictor itself starts with
        if pred.mode > 0 && pred.mode < 15 {
            return decode_error("alac: invalid mode");
        }
        let mut rec = self.0.lock().expect("alac record poisoned");
        rec.desc[channel] = ffi::SymaccelAlacDesc { mode: pred.mode as u8, lpc_order: pred.lpc_order as u8, shift: pred.shift as u8, bps: pred.bps as u8 };
        for j in 0..32 {
            rec.coeffs[channel * 32 + j] = pred.lpc_coeffs[j];
        }
        Ok(())
    }

    fn decorrelate_mid_side(&mut self, channel0: usize, channel1: usize, _out0: &mut [i32], _out1: &mut [i32], weight: i32, shift: u8) {
        let mut rec = self.0.lock().expect("alac record poisoned");
        rec.pairs.push(AlacPair { plane0: channel0, plane1: channel1, weight, shift });
    }

    fn append_tail_bits(&mut self, channel0: usize, channel1: Option<usize>, shift: u8, tail_bits: &[u16], _out0: &mut [i32], _out1: Option<&mut [i32]>) {
        let mut rec = self.0.lock().expect("alac record poisoned");
        rec.tails.push(AlacTail { plane0: channel0, plane1: channel1, shift, bits: tail_bits.to_vec() });
    }

    fn left_justify(&mut self, shift: u32, _buf: &mut AudioBuffer<i32>) {
        let mut rec = self.0.lock().expect("alac record poisoned");
        rec.out_shift = shift;
    }
}

/// `AlacFrontEnd` over the reference's own decoder with the recording backend installed: element parsing and the adaptive
/// Golomb-Rice decoder are symphonia-codec-alac's code, unmodified.
pub struct SeamFrontEnd {
    dec: AlacDecoder,
    rec: Arc<Mutex<AlacRecord>>,
    nch: usize,
    max_frames: usize,
}

impl SeamFrontEnd {
    pub fn try_new(params: &AudioCodecParameters, opts: &AudioDecoderOptions) -> Result<Self> {
        let rec: Arc<Mutex<AlacRecord>> = Arc::new(Mutex::new(AlacRecord::default()));
        let dec = AlacDecoder::try_new_with_backend(params, opts, Box::new(Recorder(rec.clone())))?;
        // the decoder has accepted the magic cookie; its buffer is sized for the cookie's frame length (lib.rs:288-298)
        let cookie = match &params.extra_data {
            Some(extra_data) => MagicCookie::read(extra_data)?,
            None => return unsupported_error("alac: missing extra data"),
        };
        Ok(SeamFrontEnd { dec, rec, nch: usize::from(cookie.num_channels), max_frames: cookie.frame_length as usize })
    }
}

impl AlacFrontEnd for SeamFrontEnd {
    fn params(&self) -> &AudioCodecParameters {
        self.dec.codec_params()
    }

    fn channels(&self) -> usize {
        self.nch
    }

    fn max_frames(&self) -> usize {
        self.max_frames
    }

    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedAlac> {
        self.rec.lock().expect("alac record poisoned").begin_packet(self.nch);
        let planes = match self.dec.decode_ref(packet)? {
            GenericAudioBufferRef::S32(planes) => planes,
            _ => return decode_error("alac: the front end's buffer is not 32-bit"),
        };
        let frames = planes.frames();
        let mut words = Vec::with_capacity(self.nch * frames);
        for c in 0..self.nch {
            match planes.plane(c) {
                Some(plane) => words.extend_from_slice(plane),
                None => return decode_error("alac: missing audio plane"),
            }
        }
        let rec = self.rec.lock().expect("alac record poisoned");
        Ok(ParsedAlac {
            frames,
            words,
            desc: rec.desc.clone(),
            coeffs: rec.coeffs.clone(),
            pairs: rec.pairs.clone(),
            tails: rec.tails.clone(),
            out_shift: rec.out_shift,
        })
    }
}

pub struct AlacBatch {
    ctx: Context,
    front: Box<dyn AlacFrontEnd>,
    nch: usize,
    words: Pinned<i32>,                 // [packet][plane][stride]
    desc: Vec<ffi::SymaccelAlacDesc>,   // [packet][plane]
    coeffs: Vec<i32>,                   // [packet][plane][32]
    // the cross-stream batcher (SYMACCEL_BATCH_ALAC_PREDICT: a chain is an element channel, units = the stream's frame length) through
    // the slot cycle of ctx.rs: what follows the predictor is applied to a batch that came through it in place, in the page-locked slot
    slots: SlotCycle<AlacIndex>,
    buf: AudioBuffer<i32>,
    // the batches submitted with their words as i16 (every word fits: ctx.rs narrow_words) and as i32
    narrow_batches: usize,
    wide_batches: usize,
    // the rows sent with a width of their own (SYMACCEL_NARROW_INPUT=2: ctx.rs pack_rows) at 2, 3 and 4 bytes a word
    rows_sent: [usize; 3],
}

/// Where `publish` finds a packet in its batch, and what is left to do to it.
pub struct AlacIndex {
    stride: usize,  // words per element-channel slot (direct: the batch's longest packet; through the batcher: the stream's frame length)
    lens: Vec<usize>,
    pairs: Vec<Vec<AlacPair>>,
    tails: Vec<Vec<AlacTail>>,
    shifts: Vec<u32>,
}

const NO_DESC: ffi::SymaccelAlacDesc = ffi::SymaccelAlacDesc { mode: 0, lpc_order: 0, shift: 0, bps: 32 };

impl AlacBatch {
    fn index_of(batch: &[ParsedAlac], stride: usize) -> AlacIndex {
        AlacIndex {
            stride,
            lens: batch.iter().map(|p| p.frames).collect(),
            pairs: batch.iter().map(|p| p.pairs.clone()).collect(),
            tails: batch.iter().map(|p| p.tails.clone()).collect(),
            shifts: batch.iter().map(|p| p.out_shift).collect(),
        }
    }
}

impl BatchCodec for AlacBatch {
    type Parsed = ParsedAlac;

    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedAlac> {
        let p = self.front.parse(packet)?;
        if p.frames > self.front.max_frames() {
            return decode_error("alac: frame length outside the stream's bounds");
        }
        Ok(p)
    }

    fn transform(&mut self, batch: &[ParsedAlac]) -> Result<()> {
        // Packets may differ in length (the last one of a stream): every element channel gets a slot of the batch's longest
        // packet, zero-padded -- predicting the padding is harmless, it is never read back.
        let (k, nch) = (batch.len(), self.nch);
        let stride = batch.iter().map(|p| p.frames).max().unwrap_or(0);
        // (a batch that came through the batcher is done with: this one is published from `words`)
        self.slots.start_direct(Self::index_of(batch, stride));
        let words = self.words.as_mut_slice();
        place_rows(words, batch, nch, stride, 0, |p| p.words.as_slice());
        place_rows(&mut self.desc, batch, nch, 1, NO_DESC, |p| p.desc.as_slice());
        place_rows(&mut self.coeffs, batch, nch, 32, 0, |p| p.coeffs.as_slice());
        if stride == 0 {
            return Ok(());
        }
        // SAFETY: `words`, `desc` and `coeffs` cover k * nch element channels of `stride` words (sized for max_batch packets of
        // the stream's frame length).
        check(
            unsafe { ffi::symaccel_alac_predict(self.ctx.raw(), words.as_mut_ptr(), self.desc.as_ptr(), self.coeffs.as_ptr(), k * nch, stride) },
            self.ctx.raw(),
        )
    }

    fn publish(&mut self, i: usize) {
        // the predicted element channels: in the batcher's slot (in place: the result plane IS input plane 0), or in this decoder's buffer
        let (ix, slot) = self.slots.parts_mut();
        let words: &mut [i32] = match slot {
            Some(slot) => slot.out_mut::<i32>(),
            None => self.words.as_mut_slice(),
        };
        let (n, stride) = (ix.lens[i], ix.stride);
        self.buf.clear();
        self.buf.render_uninit(Some(n));
        let base = i * self.nch * stride;
        // what follows the predictor, in the decoder's order (lib.rs:541-598, 409-414), on this packet's slots
        for pair in &ix.pairs[i] {
            for t in 0..n {
                let s0 = words[base + pair.plane0 * stride + t];
                let s1 = words[base + pair.plane1 * stride + t];
                let left = s0 + s1 - ((s1 * pair.weight) >> pair.shift); // lib.rs:668-669
                words[base + pair.plane0 * stride + t] = left;
                words[base + pair.plane1 * stride + t] = left - s1;
            }
        }
        for tail in &ix.tails[i] {
            for t in 0..n {
                match tail.plane1 {
                    Some(plane1) => {
                        let a = base + tail.plane0 * stride + t;
                        let b = base + plane1 * stride + t;
                        words[a] = (words[a] << tail.shift) | tail.bits[2 * t] as i32;
                        words[b] = (words[b] << tail.shift) | tail.bits[2 * t + 1] as i32;
                    }
                    None => {
                        let a = base + tail.plane0 * stride + t;
                        words[a] = (words[a] << tail.shift) | tail.bits[t] as i32;
                    }
                }
            }
        }
        let shift = ix.shifts[i];
        for c in 0..self.nch {
            if let Some(plane) = self.buf.plane_mut(c) {
                for t in 0..n {
                    plane[t] = words[base + c * stride + t].wrapping_shl(shift);
                }
            }
        }
    }

    fn reset_state(&mut self) {}

    fn clear(&mut self) {
        self.buf.clear();
    }

    fn pooled(&self) -> bool {
        self.slots.pooled()
    }

    /// The stream's next batch goes to the process-wide batcher: residuals, predictors and coefficients are written straight into a
    /// page-locked slot; the device predicts in place, in one launch with the other streams' batches.
    fn submit(&mut self, batch: &[ParsedAlac]) -> Result<()> {
        let (k, nch) = (batch.len(), self.nch);
        let stride = self.front.max_frames(); // (the same for every batch of the stream: the group key)
        if k == 0 || stride == 0 {
            return unsupported_error("alac: an empty batch, or empty packets");
        }
        // a batch whose every word fits i16 goes up as i16 (the gather of the launch widens it); per batch
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
        self.slots.submit_io(ffi::SYMACCEL_BATCH_ALAC_PREDICT as i32, 0, k * nch, stride, in_fmt, Self::index_of(batch, stride), |slot| {
            if let Some(r) = &rows {
                r.place(slot.input::<u8>(0), stride);
                slot.input::<u8>(5).copy_from_slice(r.widths.as_slice());
            } else {
                match &packed {
                    Some(rows) => place_rows(slot.input::<i16>(0), rows, nch, stride, 0, |r| r.as_slice()),
                    None => place_rows(slot.input::<i32>(0), batch, nch, stride, 0, |p| p.words.as_slice()),
                }
            }
            place_rows(slot.input::<ffi::SymaccelAlacDesc>(1), batch, nch, 1, NO_DESC, |p| p.desc.as_slice());
            place_rows(slot.input::<i32>(2), batch, nch, 32, 0, |p| p.coeffs.as_slice());
            Ok(())
        })
    }

    fn collect(&mut self) -> Result<()> {
        self.slots.collect(|_| {})
    }

    fn hint(&mut self) {
        self.slots.hint();
    }

    fn abandon(&mut self) {
        self.slots.abandon();
    }
}

impl DecoderBatch for AlacBatch {
    fn buffer(&self) -> GenericAudioBufferRef<'_> {
        self.buf.as_generic_audio_buffer_ref()
    }
}

crate::hip_decoder!(
    HipAlacDecoder,
    AlacBatch,
    ParsedAlac,
    &[support_audio_codec!(CODEC_ID_ALAC, "alac", "Apple Lossless Audio Codec (MI355X predictors)")],
    "ALAC decoder with the same observable behaviour as `symphonia_codec_alac::AlacDecoder`."
);
crate::hip_decoder!(@new HipAlacDecoder, crate::frontends::alac_front_end, Box<dyn AlacFrontEnd>);

impl HipAlacDecoder {
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
        _opts: &AudioDecoderOptions,
        front: Box<dyn AlacFrontEnd>,
        max_batch: usize,
        pool: Option<Arc<Pool>>,
    ) -> Result<Self> {
        let params = front.params().clone();
        let (Some(rate), Some(channels)) = (params.sample_rate, params.channels.clone()) else {
            return unsupported_error("alac: sample rate and channels are required");
        };
        let nch = front.channels();
        let max_batch = max_batch.max(1);
        let max_frames = front.max_frames();
        Ok(HipAlacDecoder {
            params,
            batch: AlacBatch {
                ctx: Context::new(0)?,
                front,
                nch,
                words: Pinned::new(max_batch * nch * max_frames)?,
                desc: vec![NO_DESC; max_batch * nch],
                coeffs: vec![0; max_batch * nch * 32],
                slots: SlotCycle::new(pool, AlacBatch::index_of(&[], max_frames)),
                buf: AudioBuffer::new(AudioSpec::new(rate, channels), max_frames),
                narrow_batches: 0,
                wide_batches: 0,
                rows_sent: [0; 3],
            },
            la: Lookahead::new(max_batch),
        })
    }
}
