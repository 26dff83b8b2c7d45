//! `HipPcmDecoder`: symphonia-codec-pcm's `PcmDecoder` (lib.rs) with `decode_inner` on the MI355X.  `pcm_shape` makes the checks of
//! `PcmDecoder::try_new` (lib.rs:220-316) in their order with their error variants, then refuses what the device decoder leaves to the
//! decoder below (more than 8 channels, a coded width of 0); `parse` counts a packet's whole frames (lib.rs:320: a trailing partial frame
//! is dropped, an empty packet is 0 frames, no packet fails); `transform` / `submit` hand a whole look-ahead batch to
//! `symaccel_pcm_decode` or to the cross-stream batcher (`SYMACCEL_BATCH_PCM_DECODE`: a chain is a packet; its slots through
//! `SlotCycle`, ctx.rs) as ONE call: every packet is a row of `units` frames, the frames of the batch's longest packet, a shorter one
//! followed by zero bytes -- streams cut their packets to one size, so the batches of every stream of one shape meet in the same launches; `publish` copies a packet's planes into a
//! `GenericAudioBuffer` of the reference's variant (lib.rs:248-262).  `register` enters the decoder at `Tier::Preferred` for the twenty
//! ids.  No seam patch and no `frontends.rs` entry are needed: there is no host front end.
use std::sync::Arc;

use symphonia_core::audio::sample::{i24, u24, SampleFormat};
use symphonia_core::audio::{AsGenericAudioBufferRef, AudioSpec, Channels, GenericAudioBuffer, GenericAudioBufferRef};
use symphonia_core::codecs::audio::well_known::{
    CODEC_ID_PCM_ALAW, CODEC_ID_PCM_F32BE, CODEC_ID_PCM_F32LE, CODEC_ID_PCM_F64BE, CODEC_ID_PCM_F64LE, CODEC_ID_PCM_MULAW, CODEC_ID_PCM_S16BE,
    CODEC_ID_PCM_S16LE, CODEC_ID_PCM_S24BE, CODEC_ID_PCM_S24LE, CODEC_ID_PCM_S32BE, CODEC_ID_PCM_S32LE, CODEC_ID_PCM_S8, CODEC_ID_PCM_U16BE,
    CODEC_ID_PCM_U16LE, CODEC_ID_PCM_U24BE, CODEC_ID_PCM_U24LE, CODEC_ID_PCM_U32BE, CODEC_ID_PCM_U32LE, CODEC_ID_PCM_U8,
};
use symphonia_core::codecs::audio::{AudioCodecParameters, AudioDecoderOptions};
use symphonia_core::codecs::registry::CodecRegistry;
use symphonia_core::errors::{decode_error, unsupported_error, Result};
use symphonia_core::packet::PacketRef;
use symphonia_core::support_audio_codec;

use crate::ctx::{check, Context, Pool, SlotCycle};
use crate::decoder::DecoderBatch;
use crate::ffi;
use crate::lookahead::{BatchCodec, Lookahead};
use crate::pcmdec::PcmCodec;

/// What `try_new` makes of the codec parameters.  Stands where the other decoders have their front end.
pub struct PcmShape {
    pub codec: PcmCodec,
    pub format: SampleFormat,
    pub channels: usize,
    pub shift: u32,
    pub coded_bytes: usize,
    pub native_bytes: usize,
    pub capacity: usize,
    pub rate: u32,
    pub layout: Channels,
}

/// lib.rs:220-316, check by check, then the device decoder's own refusals.
pub fn pcm_shape(params: &AudioCodecParameters, _opts: &AudioDecoderOptions) -> Result<PcmShape> {
    let codec = match PcmCodec::from_id(params.codec) {
        Some(codec) => codec,
        None => return unsupported_error("pcm: invalid codec"),
    };
    let rate = match params.sample_rate {
        Some(rate) => rate,
        _ => return unsupported_error("pcm: sample rate is required"),
    };
    let layout = match &params.channels {
        Some(channels) => {
            if channels.count() < 1 {
                return unsupported_error("pcm: number of channels cannot be 0");
            }
            channels.clone()
        }
        None => return unsupported_error("pcm: channels or channel_layout is required"),
    };
    let capacity = params.max_frames_per_packet.unwrap_or(0) as usize;
    // lib.rs:248-262
    let (format, width) = match codec {
        PcmCodec::S32Le | PcmCodec::S32Be => (SampleFormat::S32, 32),
        PcmCodec::S24Le | PcmCodec::S24Be => (SampleFormat::S24, 24),
        PcmCodec::S16Le | PcmCodec::S16Be => (SampleFormat::S16, 16),
        PcmCodec::S8 => (SampleFormat::S8, 8),
        PcmCodec::U32Le | PcmCodec::U32Be => (SampleFormat::U32, 32),
        PcmCodec::U24Le | PcmCodec::U24Be => (SampleFormat::U24, 24),
        PcmCodec::U16Le | PcmCodec::U16Be => (SampleFormat::U16, 16),
        PcmCodec::U8 => (SampleFormat::U8, 8),
        PcmCodec::F32Le | PcmCodec::F32Be => (SampleFormat::F32, 32),
        PcmCodec::F64Le | PcmCodec::F64Be => (SampleFormat::F64, 64),
        PcmCodec::ALaw | PcmCodec::MuLaw => (SampleFormat::S16, 16),
    };
    if let Some(bits_per_coded_sample) = params.bits_per_coded_sample {
        if bits_per_coded_sample > width {
            return decode_error("pcm: bits per coded sample greater-than sample format");
        }
    }
    if let Some(bits_per_sample) = params.bits_per_sample {
        if bits_per_sample > width {
            return decode_error("pcm: bits per sample is greater-than sample format");
        }
        if let Some(bits_per_coded_sample) = params.bits_per_coded_sample {
            if bits_per_coded_sample > bits_per_sample {
                return decode_error("pcm: bits per coded sample greater-than bits per sample");
            }
        }
    }
    let decoded_width = params.bits_per_sample.unwrap_or(width);
    let coded_width = params.bits_per_coded_sample.unwrap_or(decoded_width);
    let implicit = match codec {
        PcmCodec::F32Le | PcmCodec::F32Be | PcmCodec::F64Le | PcmCodec::F64Be | PcmCodec::ALaw | PcmCodec::MuLaw => true,
        _ => false,
    };
    if implicit {
        if decoded_width != width {
            return decode_error("pcm: unexpected bits per sample");
        }
        if coded_width != width {
            return decode_error("pcm: unexpected bits per coded sample");
        }
    }
    let shift = decoded_width - coded_width;
    let channels = layout.count();
    // what symaccel_pcm_decode answers with SYMACCEL_ERR_UNSUPPORTED: these streams belong to the decoder below
    if channels > 8 || (!implicit && shift == width) {
        return unsupported_error("pcm: a shape the device decoder leaves to the decoder below");
    }
    Ok(PcmShape { codec, format, channels, shift, coded_bytes: codec.coded_bytes(), native_bytes: codec.native_bytes(), capacity, rate, layout })
}

/// One packet: its whole frames.
pub struct ParsedPcm {
    pub frames: usize,
    pub data: Vec<u8>,
}

pub struct PcmBatch {
    ctx: Context,
    shape: PcmShape,
    rows: Vec<u8>,       // the packets of the current batch, `units` frames each, zero bytes behind a shorter one
    pcm: Vec<u8>,        // [packet][channel][units] native samples
    // the cross-stream batcher through the slot cycle of ctx.rs: the PCM of a batch that came through it is read in its page-locked slot
    slots: SlotCycle<PcmIndex>,
    buf: GenericAudioBuffer,
}

/// Where `publish` finds a packet in its batch.
pub struct PcmIndex {
    units: usize,        // frames every packet of the batch occupies
    frames: Vec<usize>,  // frames of each packet of the batch
}

/// plane[f] of every channel of `$buf` from the native bytes of packet `$i`
macro_rules! pcm_fill {
    ($buf:expr, $pcm:expr, $i:expr, $nch:expr, $units:expr, $frames:expr, $nb:expr, $conv:expr) => {{
        $buf.clear();
        $buf.grow_capacity($frames);
        $buf.render_uninit(Some($frames));
        for c in 0..$nch {
            if let Some(plane) = $buf.plane_mut(c) {
                let at = ($i * $nch + c) * $units * $nb;
                for f in 0..$frames {
                    plane[f] = $conv(&$pcm[at + f * $nb..at + (f + 1) * $nb]);
                }
            }
        }
    }};
}

impl PcmBatch {
    fn param(&self) -> i32 {
        self.shape.codec.raw() | ((self.shape.channels as i32) << 8) | ((self.shape.shift as i32) << 16)
    }

    /// `units`: the frames of the batch's longest packet.
    fn index_of(batch: &[ParsedPcm]) -> PcmIndex {
        PcmIndex { units: batch.iter().map(|p| p.frames).max().unwrap_or(0), frames: batch.iter().map(|p| p.frames).collect() }
    }

    fn place(rows: &mut [u8], batch: &[ParsedPcm], pitch: usize) {
        for (i, p) in batch.iter().enumerate() {
            let row = &mut rows[i * pitch..(i + 1) * pitch];
            row[..p.data.len()].copy_from_slice(&p.data);
            for b in row[p.data.len()..].iter_mut() {
                *b = 0;
            }
        }
    }
}

impl BatchCodec for PcmBatch {
    type Parsed = ParsedPcm;

    /// lib.rs:320: the complete frames of the packet; nothing can fail (lib.rs:328 discards the render's Result).
    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedPcm> {
        let frame = self.shape.coded_bytes * self.shape.channels;
        let data: &[u8] = &packet.data;
        let frames = data.len() / frame;
        Ok(ParsedPcm { frames, data: data[..frames * frame].to_vec() })
    }

    fn transform(&mut self, batch: &[ParsedPcm]) -> Result<()> {
        let (nch, fb) = (self.shape.channels, self.shape.coded_bytes * self.shape.channels);
        let index = Self::index_of(batch);
        let units = index.units;
        self.slots.start_direct(index);
        self.rows.clear();
        self.rows.resize(batch.len() * units * fb, 0u8);
        Self::place(&mut self.rows, batch, units * fb);
        self.pcm.clear();
        self.pcm.resize(batch.len() * nch * units * self.shape.native_bytes, 0u8);
        if batch.is_empty() || units == 0 {
            return Ok(());
        }
        // SAFETY: `rows` holds the batch's packets at a pitch of `units` frames, `pcm` was sized for their planes above.
        let st = unsafe {
            ffi::symaccel_pcm_decode(self.ctx.raw(), self.rows.as_ptr() as *const core::ffi::c_void, units * fb, batch.len(), self.shape.codec.raw(), nch, self.shape.shift, units,
                                     self.pcm.as_mut_ptr() as *mut core::ffi::c_void, 0)
        };
        check(st, self.ctx.raw())
    }

    fn publish(&mut self, i: usize) {
        let ix = self.slots.index();
        let (nch, nb, units, frames) = (self.shape.channels, self.shape.native_bytes, ix.units, ix.frames[i]);
        let pcm: &[u8] = self.slots.out::<u8>().unwrap_or(self.pcm.as_slice());
        match &mut self.buf {
            GenericAudioBuffer::U8(buf) => pcm_fill!(buf, pcm, i, nch, units, frames, nb, |b: &[u8]| b[0]),
            GenericAudioBuffer::U16(buf) => pcm_fill!(buf, pcm, i, nch, units, frames, nb, |b: &[u8]| u16::from_ne_bytes([b[0], b[1]])),
            GenericAudioBuffer::U24(buf) => pcm_fill!(buf, pcm, i, nch, units, frames, nb, |b: &[u8]| u24::from(u32::from_ne_bytes([b[0], b[1], b[2], b[3]]))),
            GenericAudioBuffer::U32(buf) => pcm_fill!(buf, pcm, i, nch, units, frames, nb, |b: &[u8]| u32::from_ne_bytes([b[0], b[1], b[2], b[3]])),
            GenericAudioBuffer::S8(buf) => pcm_fill!(buf, pcm, i, nch, units, frames, nb, |b: &[u8]| i8::from_ne_bytes([b[0]])),
            GenericAudioBuffer::S16(buf) => pcm_fill!(buf, pcm, i, nch, units, frames, nb, |b: &[u8]| i16::from_ne_bytes([b[0], b[1]])),
            GenericAudioBuffer::S24(buf) => pcm_fill!(buf, pcm, i, nch, units, frames, nb, |b: &[u8]| i24::from(i32::from_ne_bytes([b[0], b[1], b[2], b[3]]))),
            GenericAudioBuffer::S32(buf) => pcm_fill!(buf, pcm, i, nch, units, frames, nb, |b: &[u8]| i32::from_ne_bytes([b[0], b[1], b[2], b[3]])),
            GenericAudioBuffer::F32(buf) => pcm_fill!(buf, pcm, i, nch, units, frames, nb, |b: &[u8]| f32::from_ne_bytes([b[0], b[1], b[2], b[3]])),
            GenericAudioBuffer::F64(buf) => {
                pcm_fill!(buf, pcm, i, nch, units, frames, nb, |b: &[u8]| f64::from_ne_bytes([b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7]]))
            }
        }
    }

    /// No state is stored between packets (lib.rs:415-417).
    fn reset_state(&mut self) {}

    fn clear(&mut self) {
        self.buf.clear();
    }

    fn pooled(&self) -> bool {
        self.slots.pooled()
    }

    fn submit(&mut self, batch: &[ParsedPcm]) -> Result<()> {
        if batch.is_empty() {
            return unsupported_error("pcm: a batch of at least one packet");
        }
        let fb = self.shape.coded_bytes * self.shape.channels;
        let index = Self::index_of(batch);
        let (param, units) = (self.param(), index.units);
        self.slots.submit(ffi::SYMACCEL_BATCH_PCM_DECODE as i32, param, batch.len(), units, index, |slot| {
            Self::place(slot.input::<u8>(0), batch, units * fb);
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

impl DecoderBatch for PcmBatch {
    fn buffer(&self) -> GenericAudioBufferRef<'_> {
        self.buf.as_generic_audio_buffer_ref()
    }
}

crate::hip_decoder!(
    HipPcmDecoder,
    PcmBatch,
    ParsedPcm,
    // the same twenty descriptors as lib.rs:448-560, by id
    &[
        support_audio_codec!(CODEC_ID_PCM_S32LE, "pcm_s32le", "PCM Signed 32-bit Little-Endian Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_S32BE, "pcm_s32be", "PCM Signed 32-bit Big-Endian Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_S24LE, "pcm_s24le", "PCM Signed 24-bit Little-Endian Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_S24BE, "pcm_s24be", "PCM Signed 24-bit Big-Endian Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_S16LE, "pcm_s16le", "PCM Signed 16-bit Little-Endian Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_S16BE, "pcm_s16be", "PCM Signed 16-bit Big-Endian Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_S8, "pcm_s8", "PCM Signed 8-bit Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_U32LE, "pcm_u32le", "PCM Unsigned 32-bit Little-Endian Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_U32BE, "pcm_u32be", "PCM Unsigned 32-bit Big-Endian Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_U24LE, "pcm_u24le", "PCM Unsigned 24-bit Little-Endian Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_U24BE, "pcm_u24be", "PCM Unsigned 24-bit Big-Endian Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_U16LE, "pcm_u16le", "PCM Unsigned 16-bit Little-Endian Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_U16BE, "pcm_u16be", "PCM Unsigned 16-bit Big-Endian Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_U8, "pcm_u8", "PCM Unsigned 8-bit Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_F32LE, "pcm_f32le", "PCM 32-bit Little-Endian Floating Point Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_F32BE, "pcm_f32be", "PCM 32-bit Big-Endian Floating Point Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_F64LE, "pcm_f64le", "PCM 64-bit Little-Endian Floating Point Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_F64BE, "pcm_f64be", "PCM 64-bit Big-Endian Floating Point Interleaved (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_ALAW, "pcm_alaw", "PCM A-law (MI355X)"),
        support_audio_codec!(CODEC_ID_PCM_MULAW, "pcm_mulaw", "PCM Mu-law (MI355X)"),
    ],
    "PCM decoder with the same observable behaviour as `symphonia_codec_pcm::PcmDecoder`."
);
crate::hip_decoder!(@new HipPcmDecoder);

impl HipPcmDecoder {
    pub fn try_new_with_pool(params: &AudioCodecParameters, opts: &AudioDecoderOptions, max_batch: usize, pool: Option<Arc<Pool>>) -> Result<Self> {
        let shape = pcm_shape(params, opts)?;
        // lib.rs:313: a buffer of the codec's sample format
        let buf = GenericAudioBuffer::new(shape.format, AudioSpec::new(shape.rate, shape.layout.clone()), shape.capacity);
        Ok(HipPcmDecoder {
            params: params.clone(),
            batch: PcmBatch { ctx: Context::new(0)?, shape, rows: Vec::new(), pcm: Vec::new(), slots: SlotCycle::new(pool, PcmBatch::index_of(&[])), buf },
            la: Lookahead::new(max_batch.max(1)),
        })
    }
}

/// Enter `HipPcmDecoder` at `Tier::Preferred` above whatever the registry holds for the twenty PCM codecs (kept apart from `register()`,
/// whose list is the five codecs with a host front end).
pub fn register(registry: &mut CodecRegistry) {
    crate::register_one::<HipPcmDecoder>(registry, true);
}
