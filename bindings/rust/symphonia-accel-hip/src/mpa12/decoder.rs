//! `HipMpa12Decoder`: symphonia-bundle-mp3's `MpaDecoder` for Layer I and Layer II streams with everything behind the bit reader on the
//! MI355X.  The front end IS the reference's decoder, patched with the sub-band seam (bindings/rust/patches/symphonia-bundle-mp3.diff,
//! `MpaDecoder::try_new_with_subband_backend`) and given a recording `SubbandBackend`: `parse` runs it on a packet -- header, length, spec
//! and layer checks, allocation, scale factors and sample reads are the reference's code and fail with the reference's errors -- and keeps
//! what crossed the seam: 16-bit codes and one record per channel.  A packet that fails records nothing, so it contributes no unit, leaves
//! the state untouched and fails alone when its turn comes (decoder.rs:85-135).  `transform` / `submit` hand a whole look-ahead batch to
//! `symaccel_mpa12_decode` or to the cross-stream batcher (`SYMACCEL_BATCH_MPA12_DECODE`: a chain is a channel; its slots through
//! `SlotCycle`, ctx.rs); `publish` copies a packet's planes out and applies the gapless trim (decoder.rs:128-131); `reset` zeroes the
//! filterbank state (decoder.rs:152-155).
//! `register` enters the decoder at `Tier::Preferred`; shapes the device path does not take go to the decoder below (`fallback.rs`).
use std::sync::{Arc, Mutex};

use symphonia_bundle_mp3::backend::{SubbandBackend, SubbandFrame};
use symphonia_bundle_mp3::MpaDecoder;
use symphonia_core::audio::{Audio, AudioBuffer, AudioMut, AudioSpec, GenericAudioBufferRef};
use symphonia_core::codecs::audio::well_known::{CODEC_ID_MP1, CODEC_ID_MP2};
use symphonia_core::codecs::audio::{AudioCodecParameters, AudioDecoder, AudioDecoderOptions};
use symphonia_core::codecs::registry::CodecRegistry;
use symphonia_core::errors::{decode_error, unsupported_error, Result};
use symphonia_core::packet::PacketRef;
use symphonia_core::support_audio_codec;

use crate::ctx::{check, Context, Pool, SlotCycle};
use crate::decoder::DecoderBatch;
use crate::ffi;
use crate::lookahead::{BatchCodec, Lookahead};
use crate::mpa12::MpaLayer;

/// What the patched decoder handed its `SubbandBackend` for one packet.
#[derive(Default)]
pub struct Mpa12Record {
    pub layer: u8,
    pub channels: usize,
    pub frames: usize,
    pub codes: Vec<u16>, // [channel][32][n_frames]
    pub rec: Vec<u8>,    // [channel][record bytes]
    pub resets: usize,
}

/// The `SubbandBackend` handed to the reference's `MpaDecoder`: the frame is recorded as the bit reader left it, nothing is dequantised
/// or synthesised on the host.
pub struct SubbandRecorder(pub Arc<Mutex<Mpa12Record>>);

impl SubbandBackend for SubbandRecorder {
    fn decode_frame(&mut self, frame: &SubbandFrame, _out: &mut AudioBuffer<f32>) {
        let mut rec = self.0.lock().expect("mpa12 record poisoned");
        let (n, rb) = if frame.layer == 1 { (32 * 12, 64) } else { (32 * 36, 128) };
        rec.layer = frame.layer;
        rec.channels = frame.num_channels;
        rec.frames += 1;
        for ch in 0..frame.num_channels {
            rec.codes.extend_from_slice(&frame.codes[ch][..n]);
            rec.rec.extend_from_slice(&frame.rec[ch][..rb]);
        }
    }

    fn reset(&mut self) {
        self.0.lock().expect("mpa12 record poisoned").resets += 1;
    }
}

/// One packet behind the bit reader.
pub struct ParsedMpa12 {
    pub trim: (usize, usize), // frames to trim from the start / end of the decoded packet when gapless (decoder.rs:128-131)
    pub codes: Vec<u16>,      // [channel][32][n_frames]
    pub rec: Vec<u8>,         // [channel][record bytes]
}

pub struct Mpa12Batch {
    ctx: Context,
    front: MpaDecoder,
    record: Arc<Mutex<Mpa12Record>>,
    layer: MpaLayer,
    nch: usize,
    codes: Vec<u16>,   // [channel][packet of the batch][32][n_frames]
    rec: Vec<u8>,      // [channel][packet of the batch][record bytes]
    vvec: Vec<f32>,    // [channel][16][64]
    vfront: Vec<i32>,  // [channel]
    pcm: Vec<f32>,     // [channel][packet of the batch][32 * n_frames]
    status: Vec<u8>,   // [channel][packet of the batch]
    // the cross-stream batcher (ctx.rs, `SlotCycle`); the index of a batch is its packets' trims.  The PCM of a batch that came through
    // the batcher is read in its page-locked slot, its state lands in `vvec` / `vfront` at collect
    slots: SlotCycle<Vec<(usize, usize)>>,
    gapless: bool,
    buf: AudioBuffer<f32>,
}

impl Mpa12Batch {
    fn packet_samples(&self) -> usize {
        32 * self.layer.n_frames()
    }

    /// One input plane of a batch, for `symaccel_mpa12_decode` and for the batcher alike: row `c * k + i` = channel `c` of packet `i`.
    fn place<T: Copy>(rows: &mut [T], batch: &[ParsedMpa12], nch: usize, n: usize, plane: impl Fn(&ParsedMpa12) -> &[T]) {
        let k = batch.len();
        for (i, p) in batch.iter().enumerate() {
            for c in 0..nch {
                rows[(c * k + i) * n..(c * k + i + 1) * n].copy_from_slice(&plane(p)[c * n..(c + 1) * n]);
            }
        }
    }
}

impl BatchCodec for Mpa12Batch {
    type Parsed = ParsedMpa12;

    /// decoder.rs:85-127 and the layer's reads (layer1/mod.rs:80-181, layer2/mod.rs:237-371) by the reference's own code.
    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedMpa12> {
        {
            let mut rec = self.record.lock().expect("mpa12 record poisoned");
            rec.frames = 0;
            rec.codes.clear();
            rec.rec.clear();
        }
        self.front.decode_ref(packet)?;
        let rec = self.record.lock().expect("mpa12 record poisoned");
        if rec.frames != 1 || rec.layer as i32 != self.layer.raw() || rec.channels != self.nch {
            // (the reference fails a packet whose spec differs from the first one's: decoder.rs:104-106)
            return decode_error("mpa: invalid audio buffer signal spec for packet");
        }
        Ok(ParsedMpa12 { trim: (packet.trim_start.get() as usize, packet.trim_end.get() as usize), codes: rec.codes.clone(), rec: rec.rec.clone() })
    }

    fn transform(&mut self, batch: &[ParsedMpa12]) -> Result<()> {
        self.slots.start_direct(batch.iter().map(|p| p.trim).collect());
        let (k, n, rb, nch) = (batch.len(), self.packet_samples(), self.layer.record_bytes(), self.nch);
        self.codes.clear();
        self.codes.resize(nch * k * n, 0u16);
        self.rec.clear();
        self.rec.resize(nch * k * rb, 0u8);
        Self::place(&mut self.codes, batch, nch, n, |p| p.codes.as_slice());
        Self::place(&mut self.rec, batch, nch, rb, |p| p.rec.as_slice());
        self.pcm.clear();
        self.pcm.resize(nch * k * n, 0.0f32);
        self.status.clear();
        self.status.resize(nch * k, 0u8);
        if k == 0 {
            return Ok(());
        }
        // SAFETY: every buffer was sized for nch chains of k packets above; the call returns after the PCM and the state are back.
        let st = unsafe {
            ffi::symaccel_mpa12_decode(self.ctx.raw(), self.layer.raw(), self.codes.as_ptr(), self.rec.as_ptr(), self.vvec.as_mut_ptr(), self.vfront.as_mut_ptr(),
                                       self.pcm.as_mut_ptr(), self.status.as_mut_ptr(), nch, k)
        };
        check(st, self.ctx.raw())
    }

    fn publish(&mut self, i: usize) {
        let n = self.packet_samples();
        let trims = self.slots.index();
        let k = trims.len();
        self.buf.clear();
        self.buf.render_uninit(Some(n));
        let pcm: &[f32] = self.slots.out::<f32>().unwrap_or(self.pcm.as_slice());
        for c in 0..self.nch {
            let src = (c * k + i) * n;
            if let Some(plane) = self.buf.plane_mut(c) {
                plane[..n].copy_from_slice(&pcm[src..src + n]);
            }
        }
        if self.gapless {
            // decoder.rs:128-131
            self.buf.trim(trims[i].0, trims[i].1);
        }
    }

    /// decoder.rs:152-155: a fresh `State` (the backend is kept and reset), and the filterbank state this side owns
    fn reset_state(&mut self) {
        self.front.reset();
        self.vvec.fill(0.0);
        self.vfront.fill(0);
    }

    fn clear(&mut self) {
        self.buf.clear();
    }

    fn pooled(&self) -> bool {
        self.slots.pooled()
    }

    fn submit(&mut self, batch: &[ParsedMpa12]) -> Result<()> {
        if batch.is_empty() {
            return unsupported_error("mpa: a batch of at least one packet");
        }
        let (k, n, rb, nch) = (batch.len(), self.packet_samples(), self.layer.record_bytes(), self.nch);
        let trims: Vec<(usize, usize)> = batch.iter().map(|p| p.trim).collect();
        self.slots.submit(ffi::SYMACCEL_BATCH_MPA12_DECODE as i32, self.layer.raw(), nch, k, trims, |slot| {
            Self::place(slot.input::<u16>(0), batch, nch, n, |p| p.codes.as_slice());
            Self::place(slot.input::<u8>(1), batch, nch, rb, |p| p.rec.as_slice());
            slot.state::<f32>(0).copy_from_slice(&self.vvec);
            slot.state::<i32>(1).copy_from_slice(&self.vfront);
            Ok(())
        })
    }

    fn collect(&mut self) -> Result<()> {
        // the state after the batch; the PCM stays where it is
        self.slots.collect(|slot| {
            self.vvec.copy_from_slice(slot.state::<f32>(0));
            self.vfront.copy_from_slice(slot.state::<i32>(1));
        })
    }

    fn hint(&mut self) {
        self.slots.hint();
    }

    fn abandon(&mut self) {
        self.slots.abandon();
    }
}

impl DecoderBatch for Mpa12Batch {
    fn buffer(&self) -> GenericAudioBufferRef<'_> {
        self.buf.as_generic_audio_buffer_ref()
    }
}

crate::hip_decoder!(
    HipMpa12Decoder,
    Mpa12Batch,
    ParsedMpa12,
    &[
        support_audio_codec!(CODEC_ID_MP1, "mp1", "MPEG Audio Layer 1 (MI355X)"),
        support_audio_codec!(CODEC_ID_MP2, "mp2", "MPEG Audio Layer 2 (MI355X)"),
    ],
    "Layer I / Layer II decoder with the same observable behaviour as `symphonia_bundle_mp3::MpaDecoder`."
);
crate::hip_decoder!(@new HipMpa12Decoder);

impl HipMpa12Decoder {
    pub fn try_new_with_pool(params: &AudioCodecParameters, opts: &AudioDecoderOptions, max_batch: usize, pool: Option<Arc<Pool>>) -> Result<Self> {
        let layer = if params.codec == CODEC_ID_MP1 {
            MpaLayer::Layer1
        }
        else if params.codec == CODEC_ID_MP2 {
            MpaLayer::Layer2
        }
        else {
            return unsupported_error("mpa: invalid codec");
        };
        // the buffer and the state planes are made here, from the parameters (the reference makes its buffer from the first header)
        let (Some(rate), Some(channels)) = (params.sample_rate, params.channels.clone()) else {
            return unsupported_error("mpa: sample rate and channels are required");
        };
        let nch = channels.count();
        if nch < 1 || nch > 2 {
            return unsupported_error("mpa: one or two channels");
        }
        let record: Arc<Mutex<Mpa12Record>> = Arc::new(Mutex::new(Mpa12Record::default()));
        // the front end never trims: the trim of a packet is applied to what the device produced (Mpa12Batch::publish)
        let front_opts = AudioDecoderOptions { gapless: false, ..Default::default() };
        let front = MpaDecoder::try_new_with_subband_backend(params, &front_opts, Box::new(SubbandRecorder(record.clone())))?;
        let max_batch = max_batch.max(1);
        Ok(HipMpa12Decoder {
            params: params.clone(),
            batch: Mpa12Batch {
                ctx: Context::new(0)?,
                front,
                record,
                layer,
                nch,
                codes: Vec::new(),
                rec: Vec::new(),
                vvec: vec![0.0; nch * 1024],
                vfront: vec![0; nch],
                pcm: Vec::new(),
                status: Vec::new(),
                slots: SlotCycle::new(pool, Vec::new()),
                gapless: opts.gapless,
                buf: AudioBuffer::new(AudioSpec::new(rate, channels), 1152),
            },
            la: Lookahead::new(max_batch),
        })
    }
}

/// Enter `HipMpa12Decoder` at `Tier::Preferred` above whatever the registry holds for MP1 and MP2 (kept apart from `register()`, whose
/// list is the five codecs it has always had).
pub fn register(registry: &mut CodecRegistry) {
    crate::register_one::<HipMpa12Decoder>(registry, true);
}
