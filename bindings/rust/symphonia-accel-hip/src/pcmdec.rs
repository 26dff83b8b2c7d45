//! PCM and G.711 on the device: `symaccel_pcm_decode` behind a safe signature.  The twin of symphonia-codec-pcm's
//! `PcmDecoder::decode_inner` (lib.rs:318-411): a packet of `len` bytes is `len / (coded bytes * channels)` interleaved frames, a
//! trailing partial frame is dropped, and no packet can fail.
//!
//! Like ADPCM this codec needs no seam patch and no entry in `frontends.rs`: nothing is parsed and no state is carried, so the packet
//! bytes are the device's input.  This file holds the twenty codecs' names, their map from the reference's codec ids and the
//! context-level call; `decoder::HipPcmDecoder` (src/pcmdec/decoder.rs) is the `AudioDecoder` over it and `pcmdec::register` its
//! registry entry; `register()` of lib.rs keeps its list.
use symphonia_core::codecs::audio::well_known::{
    CODEC_ID_PCM_ALAW, CODEC_ID_PCM_F32BE, CODEC_ID_PCM_F32LE, CODEC_ID_PCM_F64BE, CODEC_ID_PCM_F64LE, CODEC_ID_PCM_MULAW, CODEC_ID_PCM_S16BE,
    CODEC_ID_PCM_S16LE, CODEC_ID_PCM_S24BE, CODEC_ID_PCM_S24LE, CODEC_ID_PCM_S32BE, CODEC_ID_PCM_S32LE, CODEC_ID_PCM_S8, CODEC_ID_PCM_U16BE,
    CODEC_ID_PCM_U16LE, CODEC_ID_PCM_U24BE, CODEC_ID_PCM_U24LE, CODEC_ID_PCM_U32BE, CODEC_ID_PCM_U32LE, CODEC_ID_PCM_U8,
};
use symphonia_core::codecs::audio::AudioCodecId;
use symphonia_core::errors::Result;

use crate::ctx::{check, Context};
use crate::ffi;
use crate::pcm::SampleFormat;

pub mod decoder;

pub use decoder::{pcm_shape, register, HipPcmDecoder, ParsedPcm, PcmBatch, PcmShape};

/// The `SYMACCEL_PCM_*` values, one per codec id `is_supported_pcm_codec` accepts (symphonia-codec-pcm lib.rs:183-207).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum PcmCodec {
    S32Le,
    S32Be,
    S24Le,
    S24Be,
    S16Le,
    S16Be,
    S8,
    U32Le,
    U32Be,
    U24Le,
    U24Be,
    U16Le,
    U16Be,
    U8,
    F32Le,
    F32Be,
    F64Le,
    F64Be,
    ALaw,
    MuLaw,
}

/// The twenty codecs with the reference's ids, in the order of lib.rs:186-205.
pub const PCM_CODECS: [(AudioCodecId, PcmCodec); 20] = [
    (CODEC_ID_PCM_S32LE, PcmCodec::S32Le),
    (CODEC_ID_PCM_S32BE, PcmCodec::S32Be),
    (CODEC_ID_PCM_S24LE, PcmCodec::S24Le),
    (CODEC_ID_PCM_S24BE, PcmCodec::S24Be),
    (CODEC_ID_PCM_S16LE, PcmCodec::S16Le),
    (CODEC_ID_PCM_S16BE, PcmCodec::S16Be),
    (CODEC_ID_PCM_S8, PcmCodec::S8),
    (CODEC_ID_PCM_U32LE, PcmCodec::U32Le),
    (CODEC_ID_PCM_U32BE, PcmCodec::U32Be),
    (CODEC_ID_PCM_U24LE, PcmCodec::U24Le),
    (CODEC_ID_PCM_U24BE, PcmCodec::U24Be),
    (CODEC_ID_PCM_U16LE, PcmCodec::U16Le),
    (CODEC_ID_PCM_U16BE, PcmCodec::U16Be),
    (CODEC_ID_PCM_U8, PcmCodec::U8),
    (CODEC_ID_PCM_F32LE, PcmCodec::F32Le),
    (CODEC_ID_PCM_F32BE, PcmCodec::F32Be),
    (CODEC_ID_PCM_F64LE, PcmCodec::F64Le),
    (CODEC_ID_PCM_F64BE, PcmCodec::F64Be),
    (CODEC_ID_PCM_ALAW, PcmCodec::ALaw),
    (CODEC_ID_PCM_MULAW, PcmCodec::MuLaw),
];

impl PcmCodec {
    /// The codec of a reference codec id, or `None` for an id the reference's decoder does not take either.
    pub fn from_id(id: AudioCodecId) -> Option<PcmCodec> {
        for (known, codec) in PCM_CODECS.iter() {
            if *known == id {
                return Some(*codec);
            }
        }
        None
    }

    /// The value the C ABI knows the codec by.
    pub fn raw(self) -> i32 {
        let v = match self {
            PcmCodec::S32Le => ffi::SYMACCEL_PCM_S32LE,
            PcmCodec::S32Be => ffi::SYMACCEL_PCM_S32BE,
            PcmCodec::S24Le => ffi::SYMACCEL_PCM_S24LE,
            PcmCodec::S24Be => ffi::SYMACCEL_PCM_S24BE,
            PcmCodec::S16Le => ffi::SYMACCEL_PCM_S16LE,
            PcmCodec::S16Be => ffi::SYMACCEL_PCM_S16BE,
            PcmCodec::S8 => ffi::SYMACCEL_PCM_S8,
            PcmCodec::U32Le => ffi::SYMACCEL_PCM_U32LE,
            PcmCodec::U32Be => ffi::SYMACCEL_PCM_U32BE,
            PcmCodec::U24Le => ffi::SYMACCEL_PCM_U24LE,
            PcmCodec::U24Be => ffi::SYMACCEL_PCM_U24BE,
            PcmCodec::U16Le => ffi::SYMACCEL_PCM_U16LE,
            PcmCodec::U16Be => ffi::SYMACCEL_PCM_U16BE,
            PcmCodec::U8 => ffi::SYMACCEL_PCM_U8,
            PcmCodec::F32Le => ffi::SYMACCEL_PCM_F32LE,
            PcmCodec::F32Be => ffi::SYMACCEL_PCM_F32BE,
            PcmCodec::F64Le => ffi::SYMACCEL_PCM_F64LE,
            PcmCodec::F64Be => ffi::SYMACCEL_PCM_F64BE,
            PcmCodec::ALaw => ffi::SYMACCEL_PCM_ALAW,
            PcmCodec::MuLaw => ffi::SYMACCEL_PCM_MULAW,
        };
        v as i32
    }

    /// Bytes of a coded sample: 1, 2, 3, 4 or 8.
    pub fn coded_bytes(self) -> usize {
        // SAFETY: pure arithmetic on its argument.
        unsafe { ffi::symaccel_pcm_coded_bytes(self.raw()) }
    }

    /// Bytes of a sample of the reference's buffer as Rust holds it: 1, 2, 4 (i24 / u24: a 32-bit word) or 8.
    pub fn native_bytes(self) -> usize {
        // SAFETY: pure arithmetic on its argument.
        unsafe { ffi::symaccel_pcm_native_bytes(self.raw()) }
    }
}

impl Context {
    /// One packet: `bytes.len() / (coded bytes * channels)` frames (lib.rs:320; a trailing partial frame is dropped) into `out` as the
    /// native planes `[channel][frame]`, `native_bytes()` a sample.  Returns the frame count.  `Err(Unsupported)` for the shapes left
    /// to the decoder below: no channels or more than 8, a shift of the format's whole width, a shift on a float or log codec.
    /// Panics (the reference's assert! class) if `out` does not cover the planes.
    pub fn pcm_decode(&mut self, codec: PcmCodec, channels: usize, shift: u32, bytes: &[u8], out: &mut [u8]) -> Result<usize> {
        self.pcm_decode_call(codec, channels, shift, bytes, 0, codec.native_bytes(), out)
    }

    /// The same with the PCM delivered as `[frame][channel]` samples of `format`: the reference's `FromSample` of every native sample.
    pub fn pcm_decode_as(&mut self, codec: PcmCodec, channels: usize, shift: u32, bytes: &[u8], format: SampleFormat, out: &mut [u8]) -> Result<usize> {
        self.pcm_decode_call(codec, channels, shift, bytes, format.raw(), format.bytes(), out)
    }

    fn pcm_decode_call(&mut self, codec: PcmCodec, channels: usize, shift: u32, bytes: &[u8], out_fmt: i32, sample_bytes: usize, out: &mut [u8]) -> Result<usize> {
        let frame = codec.coded_bytes() * channels;
        let frames = if frame == 0 { 0 } else { bytes.len() / frame };
        assert!(out.len() >= frames * channels * sample_bytes);
        // SAFETY: the slices cover what the call reads and writes (checked above); `&mut self` is the external synchronisation
        // the context asks for.
        let st = unsafe {
            ffi::symaccel_pcm_decode(self.raw(), bytes.as_ptr() as *const core::ffi::c_void, bytes.len(), 1, codec.raw(), channels, shift, frames,
                                     out.as_mut_ptr() as *mut core::ffi::c_void, out_fmt)
        };
        check(st, self.raw())?;
        Ok(frames)
    }
}
