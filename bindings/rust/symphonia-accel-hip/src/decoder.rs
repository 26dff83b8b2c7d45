//! The decoder struct and its `AudioDecoder` / `RegisterableAudioDecoder` impls, once, for all eight decoders of the crate.
//!
//! A codec module supplies a `BatchCodec` (parse one packet on the CPU, transform a batch on the GPU, publish one packet
//! of the batch into the decoder-owned `AudioBuffer`) that also exposes that buffer; the macro wraps it in a struct
//! with the trait's observable behaviour: `reset()` zeroes the carried state and drops pre-computed frames
//! (codecs/audio.rs:252-257), a failed `decode_ref` leaves the buffer cleared (:273-278), `last_decoded()` returns the
//! buffer of the last successful call (:291-297), `codec_info()` is the descriptor of the codec in use, `finalize()` is the
//! codec's (`BatchCodec::finalize_result`: FLAC with `verify` answers with the MD5 of STREAMINFO over the packets handed out, the
//! others have no checksum, like the reference's).
//!
//! The macro's `@new` arms write the constructors that only forward -- `try_new` (no batcher), `try_new_pooled` (the process-wide
//! one) and what `try_registry_new` builds with -- in one of two shapes: `(params, opts, front, max_batch)` for the five decoders
//! with a host front end (`frontends.rs`), `(params, opts, max_batch)` for the three without one (ADPCM, Layer I/II, PCM).  A codec
//! module invokes the macro once for the decoder and once for its `@new` shape, and writes `try_new_with_pool`, which is where a
//! decoder is really made.
use symphonia_core::audio::GenericAudioBufferRef;

use crate::lookahead::BatchCodec;

/// A `BatchCodec` that owns the `AudioBuffer` its `publish` fills.
pub trait DecoderBatch: BatchCodec {
    fn buffer(&self) -> GenericAudioBufferRef<'_>;
}

#[macro_export]
macro_rules! hip_decoder {
    // the constructors of a decoder behind a host front end: `$front_end(params, opts)` makes the `$front` each of them takes
    (@new $name:ident, $front_end:path, $front:ty) => {
        impl $name {
            pub fn try_new(
                params: &symphonia_core::codecs::audio::AudioCodecParameters,
                opts: &symphonia_core::codecs::audio::AudioDecoderOptions,
                front: $front,
                max_batch: usize,
            ) -> symphonia_core::errors::Result<Self> {
                Self::try_new_with_pool(params, opts, front, max_batch, None)
            }

            /// The same decoder submitting to the process-wide cross-stream batcher (`Pool::shared()`): with many streams open, the
            /// batches of all of them go to the device in one launch (csrc/batcher.cpp).
            pub fn try_new_pooled(
                params: &symphonia_core::codecs::audio::AudioCodecParameters,
                opts: &symphonia_core::codecs::audio::AudioDecoderOptions,
                front: $front,
                max_batch: usize,
            ) -> symphonia_core::errors::Result<Self> {
                Self::try_new_with_pool(params, opts, front, max_batch, Some($crate::ctx::Pool::shared()?))
            }

            fn registry_build(
                params: &symphonia_core::codecs::audio::AudioCodecParameters,
                opts: &symphonia_core::codecs::audio::AudioDecoderOptions,
            ) -> symphonia_core::errors::Result<Self> {
                $front_end(params, opts).and_then(|front| match $crate::ctx::Pool::shared() {
                    Ok(pool) => Self::try_new_with_pool(params, opts, front, $crate::DEFAULT_LOOKAHEAD, Some(pool)),
                    Err(_) => Self::try_new(params, opts, front, $crate::DEFAULT_LOOKAHEAD),
                })
            }
        }
    };
    // ... and of one without: the packet bytes go to the device as they are
    (@new $name:ident) => {
        impl $name {
            pub fn try_new(
                params: &symphonia_core::codecs::audio::AudioCodecParameters,
                opts: &symphonia_core::codecs::audio::AudioDecoderOptions,
                max_batch: usize,
            ) -> symphonia_core::errors::Result<Self> {
                Self::try_new_with_pool(params, opts, max_batch, None)
            }

            /// The same decoder submitting to the process-wide cross-stream batcher (`Pool::shared()`).
            pub fn try_new_pooled(
                params: &symphonia_core::codecs::audio::AudioCodecParameters,
                opts: &symphonia_core::codecs::audio::AudioDecoderOptions,
                max_batch: usize,
            ) -> symphonia_core::errors::Result<Self> {
                Self::try_new_with_pool(params, opts, max_batch, Some($crate::ctx::Pool::shared()?))
            }

            fn registry_build(
                params: &symphonia_core::codecs::audio::AudioCodecParameters,
                opts: &symphonia_core::codecs::audio::AudioDecoderOptions,
            ) -> symphonia_core::errors::Result<Self> {
                match $crate::ctx::Pool::shared() {
                    Ok(pool) => Self::try_new_with_pool(params, opts, $crate::DEFAULT_LOOKAHEAD, Some(pool)),
                    Err(_) => Self::try_new(params, opts, $crate::DEFAULT_LOOKAHEAD),
                }
            }
        }
    };
    // what every decoder is (`Self::registry_build` is the `@new` arm's)
    ($name:ident, $batch:ty, $parsed:ty, $codecs:expr, $doc:literal) => {
        #[doc = $doc]
        pub struct $name {
            params: symphonia_core::codecs::audio::AudioCodecParameters,
            batch: $batch,
            la: $crate::lookahead::Lookahead<$parsed>,
        }

        impl symphonia_core::codecs::audio::AudioDecoder for $name {
            fn reset(&mut self) {
                self.la.reset_with(&mut self.batch);  // (a batch still with the cross-stream batcher is given up first)
                $crate::lookahead::BatchCodec::reset_state(&mut self.batch);
            }

            fn codec_info(&self) -> &symphonia_core::codecs::CodecInfo {
                use symphonia_core::codecs::registry::RegisterableAudioDecoder;
                // the codec that is in use
                &Self::supported_codecs().iter().find(|desc| desc.id == self.params.codec).expect("codec registered in supported_codecs").info
            }

            fn codec_params(&self) -> &symphonia_core::codecs::audio::AudioCodecParameters {
                &self.params
            }

            fn decode_ref(
                &mut self,
                packet: &symphonia_core::packet::PacketRef<'_>,
            ) -> symphonia_core::errors::Result<symphonia_core::audio::GenericAudioBufferRef<'_>> {
                // (Lookahead::decode clears the buffer on every error path: codecs/audio.rs:278)
                self.la.decode(&mut self.batch, packet)?;
                Ok($crate::decoder::DecoderBatch::buffer(&self.batch))
            }

            fn finalize(&mut self) -> symphonia_core::codecs::audio::FinalizeResult {
                $crate::lookahead::BatchCodec::finalize_result(&mut self.batch)
            }

            fn last_decoded(&self) -> symphonia_core::audio::GenericAudioBufferRef<'_> {
                $crate::decoder::DecoderBatch::buffer(&self.batch)
            }
        }

        impl symphonia_core::codecs::registry::RegisterableAudioDecoder for $name {
            fn try_registry_new(
                params: &symphonia_core::codecs::audio::AudioCodecParameters,
                opts: &symphonia_core::codecs::audio::AudioDecoderOptions,
            ) -> symphonia_core::errors::Result<Box<dyn symphonia_core::codecs::audio::AudioDecoder>> {
                // The registry builds every decoder from (params, opts) alone (codecs/registry.rs:330-341): the decoders it builds
                // find each other in the process-wide `Pool` -- their look-ahead batches go to the device in common launches
                // (csrc/batcher.cpp).  Only when the pool cannot be created does a decoder batch on its own.
                // No front end, a shape the device path does not take, no device, no memory: the decoder that was registered below
                // this one takes the track.
                match Self::registry_build(params, opts) {
                    Ok(decoder) => Ok(Box::new(decoder)),
                    Err(e) => $crate::fallback::make(params, opts, e),
                }
            }

            fn supported_codecs() -> &'static [symphonia_core::codecs::registry::SupportedAudioCodec] {
                $codecs
            }
        }
    };
}
