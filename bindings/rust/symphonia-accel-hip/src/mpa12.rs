//! MPEG Layer I / Layer II on the device from what the bit reader leaves: `symaccel_mpa12_decode` behind a safe signature.  The twin of
//! the sample loops and tails of symphonia-bundle-mp3's `Layer1::decode` (layer1/mod.rs:142-194) and `Layer2::decode`
//! (layer2/mod.rs:320-384): 16-bit sample codes plus one record per channel-packet go up the link, and dequantisation, scaling and
//! `synthesis::synthesis` run in one kernel.  Header, allocation, scale-factor and sample READING stay with the reference's reader.
//!
//! `decoder::HipMpa12Decoder` (src/mpa12/decoder.rs) is the `AudioDecoder` over it -- the reference's `MpaDecoder`, patched with the
//! `SubbandBackend` seam (bindings/rust/patches/symphonia-bundle-mp3.diff), as front end --, `mpa12::register` its registry entry for
//! `CODEC_ID_MP1` / `CODEC_ID_MP2`; `register()` of lib.rs keeps its list.  This file holds the layer's names and the context-level call.
use symphonia_core::errors::Result;

use crate::ctx::{check, Context};
use crate::ffi;

pub mod decoder;

pub use decoder::{register, HipMpa12Decoder, Mpa12Batch, ParsedMpa12};

/// The `SYMACCEL_MPA_LAYER*` values (`MpegLayer::Layer1` / `Layer2`, symphonia-bundle-mp3 common.rs).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum MpaLayer {
    Layer1,
    Layer2,
}

impl MpaLayer {
    /// The value the C ABI knows the layer by.
    pub fn raw(self) -> i32 {
        let v = match self {
            MpaLayer::Layer1 => ffi::SYMACCEL_MPA_LAYER1,
            MpaLayer::Layer2 => ffi::SYMACCEL_MPA_LAYER2,
        };
        v as i32
    }

    /// Samples per sub-band of one packet and channel: 12 (layer1/mod.rs:193) or 36 (layer2/mod.rs:383).
    pub fn n_frames(self) -> usize {
        match self {
            MpaLayer::Layer1 => 12,
            MpaLayer::Layer2 => 36,
        }
    }

    /// Bytes of one channel-packet's record: `bits[32] scf[32]` or `qclass[32] scf[3][32]`.
    pub fn record_bytes(self) -> usize {
        // SAFETY: pure arithmetic on its argument.
        unsafe { ffi::symaccel_mpa12_record_bytes(self.raw()) }
    }
}

impl Context {
    /// `codes[chain][packet][32][n_frames]` and `rec[chain][packet][record_bytes]` for `n_chains` channels; `vvec` (1024 per chain) and
    /// `vfront` (one per chain) are the reference's `SynthesisState`, read at the first packet and left as after the last; `pcm`
    /// receives `[chain][packet][32 * n_frames]` and `status` one byte per channel-packet: 0, or 1 for a record out of range (such a
    /// channel-packet is decoded as if nothing were allocated).  Panics (the reference's assert! class) if the slices do not cover
    /// the batch.
    #[allow(clippy::too_many_arguments)]
    pub fn mpa12_decode(&mut self, layer: MpaLayer, n_chains: usize, codes: &[u16], rec: &[u8], vvec: &mut [f32], vfront: &mut [i32], pcm: &mut [f32],
                        status: &mut [u8]) -> Result<()> {
        let per_packet = 32 * layer.n_frames();
        assert!(n_chains > 0 && codes.len() % (n_chains * per_packet) == 0);
        let packets = codes.len() / (n_chains * per_packet);
        assert!(rec.len() >= n_chains * packets * layer.record_bytes() && vvec.len() >= n_chains * 1024 && vfront.len() >= n_chains);
        assert!(pcm.len() >= n_chains * packets * per_packet && status.len() >= n_chains * packets);
        // SAFETY: the slices cover what the call reads and writes (checked above); `&mut self` is the external synchronisation
        // the context asks for.
        let st = unsafe {
            ffi::symaccel_mpa12_decode(self.raw(), layer.raw(), codes.as_ptr(), rec.as_ptr(), vvec.as_mut_ptr(), vfront.as_mut_ptr(), pcm.as_mut_ptr(),
                                       status.as_mut_ptr(), n_chains, packets)
        };
        check(st, self.raw())
    }
}
