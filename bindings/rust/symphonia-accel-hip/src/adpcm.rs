//! ADPCM (MS, IMA WAV, IMA QT) on the device: `symaccel_adpcm_decode` behind a safe signature.  The twin of symphonia-codec-adpcm's block
//! loop (lib.rs:122-168): a packet's bytes are `block_dur / frames_per_block` blocks back to back, every block carries its own
//! predictor state, and the whole numeric decode (codec_ms.rs, codec_ima_wav.rs, codec_ima_qt.rs) runs in one kernel.
//!
//! This codec needs no seam patch and no entry in `frontends.rs`: there is no host front end -- nothing is parsed, no entropy stage
//! runs, no state plane is carried -- so the reference crate stays as it is and the packet bytes are the device's input.
//!
//! `decoder::HipAdpcmDecoder` (src/adpcm/decoder.rs) is the `AudioDecoder` over it, `adpcm::register` its registry entry; `register()` of
//! lib.rs keeps its list.  This file holds the codec's names, the block-size table and the context-level call.
use symphonia_core::errors::Result;

use crate::ctx::{check, Context};
use crate::ffi;
use crate::pcm::SampleFormat;

pub mod decoder;

pub use decoder::{adpcm_shape, register, AdpcmBatch, AdpcmShape, HipAdpcmDecoder, ParsedAdpcm};

/// The `SYMACCEL_ADPCM_*` values (CODEC_ID_ADPCM_MS / _IMA_WAV / _IMA_QT, symphonia-codec-adpcm lib.rs:108-113).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum AdpcmCodec {
    Ms,
    ImaWav,
    ImaQt,
}

impl AdpcmCodec {
    /// The value the C ABI knows the codec by.
    pub fn raw(self) -> i32 {
        let v = match self {
            AdpcmCodec::Ms => ffi::SYMACCEL_ADPCM_MS,
            AdpcmCodec::ImaWav => ffi::SYMACCEL_ADPCM_IMA_WAV,
            AdpcmCodec::ImaQt => ffi::SYMACCEL_ADPCM_IMA_QT,
        };
        v as i32
    }

    /// Bytes of one block, or `None` for a shape the device decoder refuses (it belongs to the decoder below): those where the
    /// reference leaves samples unwritten or indexes out of range, and more than two channels.
    pub fn block_bytes(self, channels: usize, frames_per_block: usize) -> Option<usize> {
        // SAFETY: pure arithmetic on its arguments.
        let n = unsafe { ffi::symaccel_adpcm_block_bytes(self.raw(), channels, frames_per_block) };
        if n == 0 {
            None
        }
        else {
            Some(n)
        }
    }
}

impl Context {
    /// `bytes` holds whole blocks back to back; `pcm` receives `[block][channel][frames_per_block]` left-justified samples and
    /// `status` one byte per block: 0, 1 (MS block predictor out of range: the reference's `Error::Unsupported`) or 2 (IMA WAV step
    /// index out of range: `Error::DecodeError`); such a block is silence.  `Err(Unsupported)` for a refused shape.  Panics (the
    /// reference's assert! class) if the slices do not cover the blocks.
    pub fn adpcm_decode(&mut self, codec: AdpcmCodec, channels: usize, frames_per_block: usize, bytes: &[u8], pcm: &mut [i32], status: &mut [u8]) -> Result<()> {
        let (n_blocks, block) = self.adpcm_blocks(codec, channels, frames_per_block, bytes)?;
        assert!(pcm.len() >= n_blocks * channels * frames_per_block && status.len() >= n_blocks);
        // SAFETY: the slices cover what the call reads and writes (checked above); `&mut self` is the external synchronisation
        // the context asks for.
        let st = unsafe {
            ffi::symaccel_adpcm_decode(self.raw(), bytes.as_ptr() as *const core::ffi::c_void, block, n_blocks, codec.raw(), channels, frames_per_block,
                                       pcm.as_mut_ptr() as *mut core::ffi::c_void, 0, status.as_mut_ptr())
        };
        check(st, self.raw())
    }

    /// The same with the PCM delivered as `[block][frame][channel]` samples of `format` (S16 is lossless: every sample is an
    /// `i16 << 16`).
    pub fn adpcm_decode_as(&mut self, codec: AdpcmCodec, channels: usize, frames_per_block: usize, bytes: &[u8], format: SampleFormat, out: &mut [u8], status: &mut [u8]) -> Result<()> {
        let (n_blocks, block) = self.adpcm_blocks(codec, channels, frames_per_block, bytes)?;
        assert!(out.len() >= n_blocks * channels * frames_per_block * format.bytes() && status.len() >= n_blocks);
        // SAFETY: as above.
        let st = unsafe {
            ffi::symaccel_adpcm_decode(self.raw(), bytes.as_ptr() as *const core::ffi::c_void, block, n_blocks, codec.raw(), channels, frames_per_block,
                                       out.as_mut_ptr() as *mut core::ffi::c_void, format.raw(), status.as_mut_ptr())
        };
        check(st, self.raw())
    }

    /// (blocks in `bytes`, bytes of a block: the pitch of the call -- an empty slice is no blocks at the block's own pitch)
    fn adpcm_blocks(&self, codec: AdpcmCodec, channels: usize, frames_per_block: usize, bytes: &[u8]) -> Result<(usize, usize)> {
        match codec.block_bytes(channels, frames_per_block) {
            Some(block) => {
                assert!(bytes.len() % block == 0);
                Ok((bytes.len() / block, block))
            }
            None => symphonia_core::errors::unsupported_error("adpcm: a shape the device decoder refuses"),
        }
    }
}
