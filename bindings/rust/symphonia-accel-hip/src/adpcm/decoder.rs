//! `HipAdpcmDecoder`: symphonia-codec-adpcm's `AdpcmDecoder` (lib.rs) with the block decoders on the MI355X.  `parse` cuts a packet into
//! its blocks and makes, per packet, the checks the reference's readers make (a packet shorter than its blocks: the I/O error of
//! `BufReader`; an MS block predictor above 6: `Unsupported`; an IMA WAV step index above 88: `DecodeError` -- whichever the reference
//! meets first), so a packet fails alone and only blocks the kernel accepts reach the device; `transform` / `submit` hand the blocks of a
//! whole look-ahead batch to `symaccel_adpcm_decode` or to the cross-stream batcher (`SYMACCEL_BATCH_ADPCM_DECODE`: a chain is a block);
//! `publish` copies a packet's blocks from `[block][channel][frame]` into the planes.  `register` enters the decoder at
//! `Tier::Preferred`.  Shapes the device decoder refuses go to the decoder below (`fallback.rs`).  No seam patch and no `frontends.rs`
//! entry are needed: there is no host front end.
use std::sync::Arc;

use symphonia_core::audio::{Audio, AudioBuffer, AudioMut, AudioSpec, Channels, GenericAudioBufferRef};
use symphonia_core::codecs::audio::well_known::{CODEC_ID_ADPCM_IMA_QT, CODEC_ID_ADPCM_IMA_WAV, CODEC_ID_ADPCM_MS};
use symphonia_core::codecs::audio::{AudioCodecParameters, AudioDecoder, AudioDecoderOptions, FinalizeResult};
use symphonia_core::codecs::registry::{CodecRegistry, RegisterableAudioDecoder, SupportedAudioCodec};
use symphonia_core::codecs::CodecInfo;
use symphonia_core::errors::{decode_error, unsupported_error, Error, Result};
use symphonia_core::packet::PacketRef;
use symphonia_core::support_audio_codec;

use crate::adpcm::AdpcmCodec;
use crate::ctx::{check, BatchSlot, Context, Pool};
use crate::decoder::DecoderBatch;
use crate::ffi;
use crate::lookahead::{BatchCodec, Lookahead};

/// What `try_new` makes of the codec parameters: the checks of symphonia-codec-adpcm lib.rs:77-120, then the shapes the device decoder
/// refuses (`AdpcmCodec::block_bytes`).  Stands where the other decoders have their front end.
pub struct AdpcmShape {
    pub codec: AdpcmCodec,
    pub channels: usize,
    pub frames_per_block: usize,
    pub block_bytes: usize,
    pub max_frames: usize,
    pub rate: u32,
    pub layout: Channels,
}

pub fn adpcm_shape(params: &AudioCodecParameters, _opts: &AudioDecoderOptions) -> Result<AdpcmShape> {
    let codec = if params.codec == CODEC_ID_ADPCM_MS {
        AdpcmCodec::Ms
    }
    else if params.codec == CODEC_ID_ADPCM_IMA_WAV {
        AdpcmCodec::ImaWav
    }
    else if params.codec == CODEC_ID_ADPCM_IMA_QT {
        AdpcmCodec::ImaQt
    }
    else {
        return unsupported_error("adpcm: invalid codec");
    };
    let max_frames = match params.max_frames_per_packet {
        Some(frames) => frames as usize,
        _ => return unsupported_error("adpcm: maximum frames per packet is required"),
    };
    let frames_per_block = match params.frames_per_block {
        Some(v) if v != 0 => v as usize,
        _ => return unsupported_error("adpcm: valid frames per block is required"),
    };
    let rate = match params.sample_rate {
        Some(rate) => rate,
        _ => return unsupported_error("adpcm: sample rate is required"),
    };
    let layout = match &params.channels {
        Some(channels) => {
            if channels.count() > 2 {
                return unsupported_error("adpcm: up to two channels are supported");
            }
            channels.clone()
        }
        None => return unsupported_error("adpcm: channels or channel_layout is required"),
    };
    let channels = layout.count();
    match codec.block_bytes(channels, frames_per_block) {
        Some(block_bytes) => Ok(AdpcmShape { codec, channels, frames_per_block, block_bytes, max_frames, rate, layout }),
        None => unsupported_error("adpcm: a shape the device decoder leaves to the decoder below"),
    }
}

/// One packet: its whole blocks, every preamble already accepted.
pub struct ParsedAdpcm {
    pub blocks: usize,
    pub data: Vec<u8>,
}

fn underrun<T>() -> Result<T> {
    // what BufReader returns when a read passes the end of the packet (io/buf_reader.rs:14-16), as `?` converts it
    Err(Error::IoError(std::io::Error::new(std::io::ErrorKind::UnexpectedEof, "buffer underrun")))
}

pub struct AdpcmBatch {
    ctx: Context,
    shape: AdpcmShape,
    bytes: Vec<u8>,     // the blocks of the current batch, back to back
    pcm: Vec<i32>,      // [block][channel][frame]
    status: Vec<u8>,
    first: Vec<usize>,  // first block of each packet of the batch
    lens: Vec<usize>,   // blocks of each packet
    pool: Option<Arc<Pool>>,
    cur: Option<BatchSlot>,
    next: Option<BatchSlot>,
    next_first: Vec<usize>,
    next_lens: Vec<usize>,
    buf: AudioBuffer<i32>,
}

impl AdpcmBatch {
    fn param(&self) -> i32 {
        self.shape.codec.raw() | ((self.shape.channels as i32) << 8)
    }
}

impl BatchCodec for AdpcmBatch {
    type Parsed = ParsedAdpcm;

    /// lib.rs:122-168 up to the first sample: the block count, and every read that can fail, in the reference's order.
    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedAdpcm> {
        let sh = &self.shape;
        let blocks = packet.block_dur().get() as usize / sh.frames_per_block;
        if blocks * sh.frames_per_block > sh.max_frames {
            return decode_error("adpcm: packet longer than the maximum frames per packet");
        }
        let data: &[u8] = &packet.data;
        for j in 0..blocks {
            let at = j * sh.block_bytes;
            let left = if data.len() > at { data.len() - at } else { 0 };
            for c in 0..sh.channels {
                match sh.codec {
                    AdpcmCodec::Ms => {
                        // codec_ms.rs:47-63: the block predictors are the first bytes, each checked as it is read
                        if left <= c {
                            return underrun();
                        }
                        if data[at + c] > 6 {
                            return unsupported_error("adpcm: block predictor exceeds range");
                        }
                    }
                    AdpcmCodec::ImaWav => {
                        // codec_ima_wav.rs:14-25: predictor (2 bytes), step index, reserved byte, channel after channel
                        if left < 4 * c + 3 {
                            return underrun();
                        }
                        if data[at + 4 * c + 2] > 88 {
                            return decode_error("adpcm (ima): invalid step index");
                        }
                        if left < 4 * c + 4 {
                            return underrun();
                        }
                    }
                    AdpcmCodec::ImaQt => {}
                }
            }
            if left < sh.block_bytes {
                return underrun();
            }
        }
        Ok(ParsedAdpcm { blocks, data: data[..blocks * sh.block_bytes].to_vec() })
    }

    fn transform(&mut self, batch: &[ParsedAdpcm]) -> Result<()> {
        if let (Some(pool), Some(old)) = (self.pool.clone(), self.cur.take()) {
            pool.release(old);
        }
        let (nch, fpb) = (self.shape.channels, self.shape.frames_per_block);
        self.bytes.clear();
        self.first.clear();
        self.lens.clear();
        let mut total = 0;
        for p in batch {
            self.first.push(total);
            self.lens.push(p.blocks);
            self.bytes.extend_from_slice(&p.data);
            total += p.blocks;
        }
        self.pcm.clear();
        self.pcm.resize(total * nch * fpb, 0i32);
        self.status.clear();
        self.status.resize(total, 0u8);
        if total == 0 {
            return Ok(());
        }
        // SAFETY: `bytes` holds `total` blocks back to back, `pcm` and `status` were sized for them above.
        let st = unsafe {
            ffi::symaccel_adpcm_decode(self.ctx.raw(), self.bytes.as_ptr() as *const core::ffi::c_void, self.shape.block_bytes, total, self.shape.codec.raw(), nch, fpb,
                                       self.pcm.as_mut_ptr() as *mut core::ffi::c_void, 0, self.status.as_mut_ptr())
        };
        check(st, self.ctx.raw())
    }

    fn publish(&mut self, i: usize) {
        let (nch, fpb) = (self.shape.channels, self.shape.frames_per_block);
        let (first, blocks) = (self.first[i], self.lens[i]);
        self.buf.clear();
        self.buf.render_uninit(Some(blocks * fpb));
        let pcm: &[i32] = match &self.cur {
            Some(slot) => slot.out::<i32>(),
            None => self.pcm.as_slice(),
        };
        for c in 0..nch {
            if let Some(plane) = self.buf.plane_mut(c) {
                for j in 0..blocks {
                    let at = ((first + j) * nch + c) * fpb;
                    plane[j * fpb..(j + 1) * fpb].copy_from_slice(&pcm[at..at + fpb]);
                }
            }
        }
    }

    /// No state is stored between packets (lib.rs:217-219).
    fn reset_state(&mut self) {}

    fn clear(&mut self) {
        self.buf.clear();
    }

    fn pooled(&self) -> bool {
        self.pool.is_some()
    }

    fn submit(&mut self, batch: &[ParsedAdpcm]) -> Result<()> {
        let Some(pool) = self.pool.clone() else {
            return unsupported_error("adpcm: no batcher");
        };
        let total: usize = batch.iter().map(|p| p.blocks).sum();
        if total == 0 || self.next.is_some() {
            return unsupported_error("adpcm: one batch of at least one block at a time");
        }
        let mut slot = pool.reserve(ffi::SYMACCEL_BATCH_ADPCM_DECODE as i32, self.param(), total, self.shape.block_bytes)?;
        self.next_first.clear();
        self.next_lens.clear();
        {
            let rows = slot.input::<u8>(0);
            let mut at = 0;
            let mut block = 0;
            for p in batch {
                rows[at..at + p.data.len()].copy_from_slice(&p.data);
                at += p.data.len();
                self.next_first.push(block);
                self.next_lens.push(p.blocks);
                block += p.blocks;
            }
        }
        if let Err(e) = pool.commit(&mut slot) {
            pool.release(slot);
            return Err(e);
        }
        self.next = Some(slot);
        Ok(())
    }

    fn collect(&mut self) -> Result<()> {
        let (Some(pool), Some(mut slot)) = (self.pool.clone(), self.next.take()) else {
            return unsupported_error("adpcm: nothing was submitted");
        };
        if let Err(e) = pool.wait(&mut slot) {
            pool.release(slot);
            return Err(e);
        }
        if let Some(old) = self.cur.take() {
            pool.release(old);
        }
        self.cur = Some(slot);
        std::mem::swap(&mut self.first, &mut self.next_first);
        std::mem::swap(&mut self.lens, &mut self.next_lens);
        Ok(())
    }

    fn hint(&mut self) {
        if let Some(pool) = &self.pool {
            pool.hint();
        }
    }

    fn abandon(&mut self) {
        if let (Some(pool), Some(slot)) = (self.pool.clone(), self.next.take()) {
            pool.release(slot);
        }
    }
}

impl Drop for AdpcmBatch {
    fn drop(&mut self) {
        BatchCodec::abandon(self);
        if let (Some(pool), Some(slot)) = (self.pool.clone(), self.cur.take()) {
            pool.release(slot);
        }
    }
}

impl DecoderBatch for AdpcmBatch {
    fn buffer(&self) -> GenericAudioBufferRef<'_> {
        self.buf.as_generic_audio_buffer_ref()
    }
}

/// ADPCM decoder with the same observable behaviour as `symphonia_codec_adpcm::AdpcmDecoder`.
pub struct HipAdpcmDecoder {
    params: AudioCodecParameters,
    batch: AdpcmBatch,
    la: Lookahead<ParsedAdpcm>,
}

impl HipAdpcmDecoder {
    pub fn try_new(params: &AudioCodecParameters, opts: &AudioDecoderOptions, max_batch: usize) -> Result<Self> {
        Self::try_new_with_pool(params, opts, max_batch, None)
    }

    /// The same decoder submitting to the process-wide cross-stream batcher (`Pool::shared()`).
    pub fn try_new_pooled(params: &AudioCodecParameters, opts: &AudioDecoderOptions, max_batch: usize) -> Result<Self> {
        Self::try_new_with_pool(params, opts, max_batch, Some(Pool::shared()?))
    }

    pub fn try_new_with_pool(params: &AudioCodecParameters, opts: &AudioDecoderOptions, max_batch: usize, pool: Option<Arc<Pool>>) -> Result<Self> {
        let shape = adpcm_shape(params, opts)?;
        let buf = AudioBuffer::new(AudioSpec::new(shape.rate, shape.layout.clone()), shape.max_frames);
        Ok(HipAdpcmDecoder {
            params: params.clone(),
            batch: AdpcmBatch {
                ctx: Context::new(0)?,
                shape,
                bytes: Vec::new(),
                pcm: Vec::new(),
                status: Vec::new(),
                first: Vec::new(),
                lens: Vec::new(),
                pool,
                cur: None,
                next: None,
                next_first: Vec::new(),
                next_lens: Vec::new(),
                buf,
            },
            la: Lookahead::new(max_batch.max(1)),
        })
    }
}

impl AudioDecoder for HipAdpcmDecoder {
    /// Nothing is carried between packets (lib.rs:217-219): only what was computed ahead is dropped.
    fn reset(&mut self) {
        self.la.reset_with(&mut self.batch);
        BatchCodec::reset_state(&mut self.batch);
    }

    fn codec_info(&self) -> &CodecInfo {
        // the codec that is in use (lib.rs:176-183)
        &Self::supported_codecs().iter().find(|desc| desc.id == self.params.codec).expect("codec registered in supported_codecs").info
    }

    fn codec_params(&self) -> &AudioCodecParameters {
        &self.params
    }

    fn decode_ref(&mut self, packet: &PacketRef<'_>) -> Result<GenericAudioBufferRef<'_>> {
        // (Lookahead::decode clears the buffer on every error path: lib.rs:190-198)
        self.la.decode(&mut self.batch, packet)?;
        Ok(DecoderBatch::buffer(&self.batch))
    }

    fn finalize(&mut self) -> FinalizeResult {
        Default::default()
    }

    fn last_decoded(&self) -> GenericAudioBufferRef<'_> {
        DecoderBatch::buffer(&self.batch)
    }
}

impl RegisterableAudioDecoder for HipAdpcmDecoder {
    fn try_registry_new(params: &AudioCodecParameters, opts: &AudioDecoderOptions) -> Result<Box<dyn AudioDecoder>> {
        // as the other decoders of this crate (decoder.rs): on the shared batcher if there is one; a shape, a device or memory this
        // decoder cannot have sends the track to the decoder that was registered below
        let built = match Pool::shared() {
            Ok(pool) => Self::try_new_with_pool(params, opts, crate::DEFAULT_LOOKAHEAD, Some(pool)),
            Err(_) => Self::try_new(params, opts, crate::DEFAULT_LOOKAHEAD),
        };
        match built {
            Ok(decoder) => Ok(Box::new(decoder)),
            Err(e) => crate::fallback::make(params, opts, e),
        }
    }

    fn supported_codecs() -> &'static [SupportedAudioCodec] {
        &[
            support_audio_codec!(CODEC_ID_ADPCM_MS, "adpcm_ms", "Microsoft ADPCM (MI355X)"),
            support_audio_codec!(CODEC_ID_ADPCM_IMA_WAV, "adpcm_ima_wav", "ADPCM IMA WAV (MI355X)"),
            support_audio_codec!(CODEC_ID_ADPCM_IMA_QT, "adpcm_ima_qt", "ADPCM IMA QT (MI355X)"),
        ]
    }
}

/// Enter `HipAdpcmDecoder` at `Tier::Preferred` above whatever the registry holds for the three ADPCM codecs (kept apart from
/// `register()`, whose list is the five codecs with a host front end).
pub fn register(registry: &mut CodecRegistry) {
    crate::register_one::<HipAdpcmDecoder>(registry, true);
}
