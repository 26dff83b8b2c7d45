//! `HipAdpcmDecoder`: symphonia-codec-adpcm's `AdpcmDecoder` (lib.rs) with the block decoders on the MI355X.  `parse` cuts a packet into
//! its blocks and makes, per packet, the checks the reference's readers make (a packet shorter than its blocks: the I/O error of
//! `BufReader`; an MS block predictor above 6: `Unsupported`; an IMA WAV step index above 88: `DecodeError` -- whichever the reference
//! meets first), so a packet fails alone and only blocks the kernel accepts reach the device; `transform` / `submit` hand the blocks of a
//! whole look-ahead batch to `symaccel_adpcm_decode` or to the cross-stream batcher (`SYMACCEL_BATCH_ADPCM_DECODE`: a chain is a block;
//! its slots through `SlotCycle`, ctx.rs); `publish` copies a packet's blocks from `[block][channel][frame]` into the planes.
//! `register` enters the decoder at `Tier::Preferred`.  Shapes the device decoder refuses go to the decoder below (`fallback.rs`).  No seam patch and no `frontends.rs`
//! entry are needed: there is no host front end.
use std::sync::Arc;

use symphonia_core::audio::{Audio, AudioBuffer, AudioMut, AudioSpec, Channels, GenericAudioBufferRef};
use symphonia_core::codecs::audio::well_known::{CODEC_ID_ADPCM_IMA_QT, CODEC_ID_ADPCM_IMA_WAV, CODEC_ID_ADPCM_MS};
use symphonia_core::codecs::audio::{AudioCodecParameters, AudioDecoderOptions};
use symphonia_core::codecs::registry::CodecRegistry;
use symphonia_core::errors::{decode_error, unsupported_error, Error, Result};
use symphonia_core::packet::PacketRef;
use symphonia_core::support_audio_codec;

use crate::adpcm::AdpcmCodec;
use crate::ctx::{check, Context, Pool, SlotCycle};
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
    // the cross-stream batcher through the slot cycle of ctx.rs: the PCM of a batch that came through it is read in its page-locked slot
    slots: SlotCycle<AdpcmIndex>,
    buf: AudioBuffer<i32>,
}

/// Where `publish` finds a packet in its batch.
pub struct AdpcmIndex {
    first: Vec<usize>,  // first block of each packet of the batch
    lens: Vec<usize>,   // blocks of each packet
    total: usize,
}

impl AdpcmBatch {
    fn param(&self) -> i32 {
        self.shape.codec.raw() | ((self.shape.channels as i32) << 8)
    }

    fn index_of(batch: &[ParsedAdpcm]) -> AdpcmIndex {
        let mut first = Vec::with_capacity(batch.len());
        let mut total = 0;
        for p in batch {
            first.push(total);
            total += p.blocks;
        }
        AdpcmIndex { first, lens: batch.iter().map(|p| p.blocks).collect(), total }
    }

    /// The blocks of a batch back to back: what `symaccel_adpcm_decode` and the batcher's slot both take.
    fn place(rows: &mut [u8], batch: &[ParsedAdpcm]) {
        let mut at = 0;
        for p in batch {
            rows[at..at + p.data.len()].copy_from_slice(&p.data);
            at += p.data.len();
        }
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
        let index = Self::index_of(batch);
        let total = index.total;
        self.slots.start_direct(index);
        let (nch, fpb) = (self.shape.channels, self.shape.frames_per_block);
        self.bytes.clear();
        self.bytes.resize(total * self.shape.block_bytes, 0u8);
        Self::place(&mut self.bytes, batch);
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
        let ix = self.slots.index();
        let (first, blocks) = (ix.first[i], ix.lens[i]);
        self.buf.clear();
        self.buf.render_uninit(Some(blocks * fpb));
        let pcm: &[i32] = self.slots.out::<i32>().unwrap_or(self.pcm.as_slice());
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
        self.slots.pooled()
    }

    fn submit(&mut self, batch: &[ParsedAdpcm]) -> Result<()> {
        let index = Self::index_of(batch);
        if index.total == 0 {
            return unsupported_error("adpcm: a batch of at least one block");
        }
        let (param, total) = (self.param(), index.total);
        self.slots.submit(ffi::SYMACCEL_BATCH_ADPCM_DECODE as i32, param, total, self.shape.block_bytes, index, |slot| {
            Self::place(slot.input::<u8>(0), batch);
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

impl DecoderBatch for AdpcmBatch {
    fn buffer(&self) -> GenericAudioBufferRef<'_> {
        self.buf.as_generic_audio_buffer_ref()
    }
}

crate::hip_decoder!(
    HipAdpcmDecoder,
    AdpcmBatch,
    ParsedAdpcm,
    &[
        support_audio_codec!(CODEC_ID_ADPCM_MS, "adpcm_ms", "Microsoft ADPCM (MI355X)"),
        support_audio_codec!(CODEC_ID_ADPCM_IMA_WAV, "adpcm_ima_wav", "ADPCM IMA WAV (MI355X)"),
        support_audio_codec!(CODEC_ID_ADPCM_IMA_QT, "adpcm_ima_qt", "ADPCM IMA QT (MI355X)"),
    ],
    "ADPCM decoder with the same observable behaviour as `symphonia_codec_adpcm::AdpcmDecoder`."
);
crate::hip_decoder!(@new HipAdpcmDecoder);

impl HipAdpcmDecoder {
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
                slots: SlotCycle::new(pool, AdpcmBatch::index_of(&[])),
                buf,
            },
            la: Lookahead::new(max_batch.max(1)),
        })
    }
}

/// Enter `HipAdpcmDecoder` at `Tier::Preferred` above whatever the registry holds for the three ADPCM codecs (kept apart from
/// `register()`, whose list is the five codecs with a host front end).
pub fn register(registry: &mut CodecRegistry) {
    crate::register_one::<HipAdpcmDecoder>(registry, true);
}
