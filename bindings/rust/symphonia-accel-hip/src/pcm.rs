//! PCM in the caller's sample format: `symaccel_pcm_convert` behind a safe signature.  The twin of
//! `GenericAudioBufferRef::copy_bytes_to_vec_interleaved_as::<S>` (symphonia-core/src/audio/generic.rs:204-340) for planes that
//! are already in host memory: the conversion (audio/conv.rs, `FromSample`) and the interleave (audio/util.rs:119-167) run on the
//! device, the result is the byte stream an audio output wants.
use symphonia_core::errors::Result;

use crate::ctx::{check, Context};
use crate::ffi;

/// The `SYMACCEL_FMT_*` values.  `S32` and `F32` are also the two source formats: the FLAC / ALAC planes (left-justified) and the
/// planes of the transform codecs.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum SampleFormat {
    U8,
    S8,
    U16,
    S16,
    U24,
    S24,
    U32,
    S32,
    F32,
}

impl SampleFormat {
    /// The value the C ABI knows the format by.
    pub fn raw(self) -> i32 {
        let v = match self {
            SampleFormat::U8 => ffi::SYMACCEL_FMT_U8,
            SampleFormat::S8 => ffi::SYMACCEL_FMT_S8,
            SampleFormat::U16 => ffi::SYMACCEL_FMT_U16,
            SampleFormat::S16 => ffi::SYMACCEL_FMT_S16,
            SampleFormat::U24 => ffi::SYMACCEL_FMT_U24,
            SampleFormat::S24 => ffi::SYMACCEL_FMT_S24,
            SampleFormat::U32 => ffi::SYMACCEL_FMT_U32,
            SampleFormat::S32 => ffi::SYMACCEL_FMT_S32,
            SampleFormat::F32 => ffi::SYMACCEL_FMT_F32,
        };
        v as i32
    }

    /// Bytes per sample; the 24-bit formats are three packed little-endian bytes.
    pub fn bytes(self) -> usize {
        // SAFETY: pure arithmetic on its argument.
        unsafe { ffi::symaccel_sample_bytes(self.raw()) }
    }
}

/// Planes the library produces: `&[f32]` or `&[i32]`, 4 bytes a sample.
pub trait SourceSample: Copy {
    const FORMAT: SampleFormat;
}

impl SourceSample for f32 {
    const FORMAT: SampleFormat = SampleFormat::F32;
}

impl SourceSample for i32 {
    const FORMAT: SampleFormat = SampleFormat::S32;
}

impl Context {
    /// `pcm_convert_f32` / `pcm_convert_i32` by the planes' own type.
    pub fn pcm_convert<S: SourceSample>(&mut self, planes: &[S], plane_stride: usize, channels: usize, n_frames: usize, format: SampleFormat, out: &mut [u8]) -> Result<()> {
        self.pcm_convert_raw(planes.as_ptr() as *const core::ffi::c_void, planes.len(), S::FORMAT, plane_stride, channels, n_frames, format, out)
    }

    /// `planes` holds `n_groups * channels` f32 planes of `plane_stride` samples, the first `n_frames` of each valid; `out` receives
    /// `[n_groups][n_frames][channels]` samples of `format`, back to back.  Panics (the reference's assert! class) if the slices do
    /// not cover that.
    pub fn pcm_convert_f32(&mut self, planes: &[f32], plane_stride: usize, channels: usize, n_frames: usize, format: SampleFormat, out: &mut [u8]) -> Result<()> {
        self.pcm_convert_raw(planes.as_ptr() as *const core::ffi::c_void, planes.len(), SampleFormat::F32, plane_stride, channels, n_frames, format, out)
    }

    /// The same for left-justified i32 planes, as the FLAC and ALAC decoders leave them.
    pub fn pcm_convert_i32(&mut self, planes: &[i32], plane_stride: usize, channels: usize, n_frames: usize, format: SampleFormat, out: &mut [u8]) -> Result<()> {
        self.pcm_convert_raw(planes.as_ptr() as *const core::ffi::c_void, planes.len(), SampleFormat::S32, plane_stride, channels, n_frames, format, out)
    }

    #[allow(clippy::too_many_arguments)]
    fn pcm_convert_raw(&mut self, planes: *const core::ffi::c_void, n_samples: usize, source: SampleFormat, plane_stride: usize, channels: usize, n_frames: usize,
                       format: SampleFormat, out: &mut [u8]) -> Result<()> {
        assert!(channels >= 1 && channels <= 8 && plane_stride >= n_frames && plane_stride > 0 && n_samples % (plane_stride * channels) == 0);
        let n_groups = n_samples / (plane_stride * channels);
        let group_bytes = n_frames * channels * format.bytes();
        assert!(out.len() >= n_groups * group_bytes);
        // SAFETY: both slices cover what the call reads and writes (checked above); `&mut self` is the external synchronisation
        // the context asks for.
        let status = unsafe {
            ffi::symaccel_pcm_convert(self.raw(), planes, source.raw(), plane_stride, n_groups, channels, n_frames, out.as_mut_ptr() as *mut core::ffi::c_void, format.raw(),
                                      group_bytes)
        };
        check(status, self.raw())
    }
}
